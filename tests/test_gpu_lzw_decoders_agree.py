"""tiff_lzw_decode_kernel (csrc/tiff_lzw.hip) and tiff_lzw_decode_chunks_kernel (csrc/tiff_read.hip) run one loop, lzw_decode_stream
(csrc/lzw_decode.h), over two sinks: on the streams that reach every branch of the stream rules and every status the loop returns,
the two give the same status and the same bytes."""
import numpy as np
import pytest
import torch

import raster_reader_cases as rc
import test_gpu_tiff_decode as td
import tiff_lzw_decode_cases as dc
from flair_amd import raster_reader as rr

pytestmark = pytest.mark.gpu


def _streams():
    """(name, stream, dst_len, mode): GOOD and the defined failures of test_gpu_tiff_decode, and the window streams of the chunk
    decoder that the strip decoder's cap admits"""
    out = [(name, enc, len(want), mode) for name, enc, want, mode in td.GOOD]
    out += [(name, stream, want, mode) for name, stream, want, mode, _ in td._bad_strips()]
    out += [(name, s, len(raw), 1) for name, (s, raw, _) in rc.window_chunks(rr.CHUNK_WINDOW).items() if len(raw) <= dc.MAX_STRIP]
    return out


def test_both_decoders_give_the_same_status_and_bytes(dev):
    from flair_amd import ops
    streams = _streams()
    assert all(1 <= n <= dc.MAX_STRIP for _, _, n, _ in streams) and sum(name.startswith("edge_") for name, *_ in streams) == 5
    parts, off, at = [], [], 0
    for _, s, _, _ in streams:                       # one source for both: every stream at an offset of 3 modulo 4
        pad = (3 - at) % 4
        parts.append(b"\xff" * pad + s)
        off.append(at + pad)
        at += pad + len(s)
    up = lambda a, dt: torch.from_numpy(np.array(a, dtype=dt)).to(dev)   # noqa: E731
    src = up(np.frombuffer(b"".join(parts) + b"\xff" * 3, np.uint8), np.uint8)
    src_off, src_len = up(off, np.int64), up([len(s) for _, s, _, _ in streams], np.int32)
    dst_len, mode = [n for _, _, n, _ in streams], up([m for _, _, _, m in streams], np.int32)

    slot = -(-max(dst_len) // rc.GUARD) * rc.GUARD   # the chunk decoder's slots: dst_len rounded up to 128
    scratch = torch.full((len(streams) * slot,), dc.FILL, dtype=torch.uint8, device=dev)
    slots, st_chunks = ops.tiff_lzw_decode_chunks(src, src_off, src_len, up(dst_len, np.int32), mode, slot, out=scratch)

    dst_off = [i * slot + 5 for i in range(len(streams))]   # the strip decoder's regions: the same pitch, an odd phase
    dst = torch.full((len(streams) * slot + 5,), dc.FILL, dtype=torch.uint8, device=dev)
    _, st_strips = ops.tiff_lzw_decode(src, src_off, src_len, up(dst_off, np.int64), up(dst_len, np.int32), mode, dst.numel(), out=dst)

    st_chunks, st_strips = st_chunks.cpu().numpy(), st_strips.cpu().numpy()
    assert st_chunks.tolist() == st_strips.tolist()
    assert set(st_strips.tolist()) == {0, 1, 2, 3, 4}
    slots, dst = slots.cpu().numpy(), dst.cpu().numpy()
    for i, (name, _, n, _) in enumerate(streams):
        # what a stream did not produce still holds the fill on both sides: equal regions are equal bytes and equal lengths
        assert slots[i, :n].tobytes() == dst[dst_off[i]:dst_off[i] + n].tobytes(), name
    assert dc.guards_intact(slots.reshape(-1), [i * slot for i in range(len(streams))], dst_len) and dc.guards_intact(dst, dst_off, dst_len)
