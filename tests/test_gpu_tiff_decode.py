"""tiff_lzw_decode_kernel (csrc/tiff_lzw.hip) through the C ABI, ops.tiff_lzw_decode, tiff.read_masks and metrics(decode="device"):
bytes and status per strip equal the reference decoder of tiff_lzw_decode_cases, nothing is written outside a strip's own region,
every defined failure gets its status, and the device mode of metrics() writes what the host mode writes."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import tiff_lzw_cases as tc
import tiff_lzw_decode_cases as dc

pytestmark = pytest.mark.gpu


def _launch(dev, strips, misalign=0, src_bytes=None):
    """one launch of (stream, dst_len, mode) strips over a 0xA5-filled dst with guards; returns (dst, status, dst_off, dst_len)"""
    from flair_amd import _lib as L
    src, src_off, src_len, dst_off, dst_len, mode, dst_bytes = dc.strip_table(strips, misalign=misalign)
    t = [torch.from_numpy(a).to(dev) for a in (src, src_off, src_len, dst_off, dst_len, mode)]
    dst = torch.full((dst_bytes,), dc.FILL, dtype=torch.uint8, device=dev)
    status = torch.full((len(strips),), -7, dtype=torch.int32, device=dev)
    rc = L.lib().flair_tiff_lzw_decode(L.ptr(t[0]), src.size if src_bytes is None else src_bytes, *(L.ptr(x) for x in t[1:]), len(strips),
                                       L.ptr(dst), dst_bytes, L.ptr(status), L.stream())
    assert rc == 0
    return dst.cpu().numpy(), status.cpu().numpy(), dst_off, dst_len


def _good_strips():
    """(name, stream, decoded bytes, mode): every branch of a well-formed stream at the smallest size that reaches it"""
    row = tc.boundary_row()
    _, lengths = tc.boundary_lengths(row)
    out = [(f"boundary_{L}", tc.lzw_strip(row[:L].tobytes()), row[:L].tobytes(), 1) for L in lengths + [1, 2, 3]]
    const = dc.constant_strip(16384)              # code == nxt on every code, strings far beyond 64 bytes, the overlapping copy
    out.append(("constant_16384", tc.lzw_strip(const), const, 1))
    for k in (19, 256):
        s = dc.values_strip(8192, k)
        out.append((f"values{k}_8192", tc.lzw_strip(s), s, 1))
    img = np.random.default_rng(11).integers(0, 19, (40, 37)).astype(np.uint8)   # 8-row strips: odd, unaligned dst_off
    out += [(f"40x37_strip{i}", s, img[8 * i:8 * i + 8].tobytes(), 1) for i, s in enumerate(tc.ref_strips(img, 8))]
    big = tc.smooth_mask()[:128].tobytes()        # exactly the cap: the large size class
    out.append(("cap_65536", tc.lzw_strip(big), big, 1))
    out.append(("small_class_edge_16385", tc.lzw_strip(big[:16385]), big[:16385], 1))
    raw = bytes(range(37))
    out.append(("stored_37", raw, raw, 0))
    s = dc.values_strip(6000, 19, seed=2)
    out.append(("clear_every_100", dc.lzw_strip_with_clears(s, 100), s, 1))
    full = dc.values_strip(12000, 256, seed=5)    # no reset: the table fills up and the stream goes on in 12-bit codes
    out.append(("full_table", dc.lzw_strip_with_clears(full, 10 ** 9, reset_at=None), full, 1))
    enc = tc.lzw_strip(s)
    out.append(("eoi_cut_off", enc[:-1], s, 1))   # EOI has 9 bits at least: the last byte holds nothing else
    out.append(("garbage_appended", enc + bytes(range(200, 216)), s, 1))
    out.append(("clipped_last_string", tc.lzw_strip(const), const[:16000], 1))
    return out


GOOD = _good_strips()


@pytest.fixture(scope="module")
def good_launch(dev):
    return _launch(dev, [(enc, len(want), mode) for _, enc, want, mode in GOOD], misalign=3)


def test_reference_decodes_every_good_strip():
    for name, enc, want, mode in GOOD:
        if mode == 1:
            assert dc.lzw_decode_strip(enc, len(want)) == (want, 0), name


@pytest.mark.parametrize("i", range(len(GOOD)), ids=[g[0] for g in GOOD])
def test_bytes_equal_the_reference_decoder(good_launch, i):
    dst, status, dst_off, dst_len = good_launch
    _, _, want, _ = GOOD[i]
    assert status[i] == 0
    got = dst[dst_off[i]:dst_off[i] + dst_len[i]].tobytes()
    assert got == want, f"first difference at byte {next(j for j, (p, q) in enumerate(zip(got, want)) if p != q)} of {len(want)}"


def test_guards_of_the_mixed_launch(good_launch):
    dst, status, dst_off, dst_len = good_launch
    assert len({int(o) % 16 for o in dst_off}) > 4          # regions start at many alignments
    assert dc.guards_intact(dst, dst_off, dst_len) and (status == 0).all()


@pytest.mark.parametrize("shape", [(64, 96), (40, 37), (512, 512)])
def test_pil_files_through_read_masks(dev, tmp_path, shape):
    from flair_amd.tiff import read_masks, tiff_strip_layout
    img = tc.smooth_mask() if shape == (512, 512) else dc.small_image(*shape)
    paths = []
    for kind, kw in (("lzw", {"compression": "tiff_lzw"}), ("stored", {})):
        paths.append(tmp_path / f"{kind}.tif")
        Image.fromarray(img).save(paths[-1], **kw)
    lay = tiff_strip_layout(paths[0].read_bytes())
    assert lay is not None and (lay.H, lay.W) == shape and len(lay.offsets) == (4 if shape == (512, 512) else 1)
    reads = read_masks(paths, dev, "device")
    for r, p in zip(reads, paths):
        assert r.where == "device" and r.error is None and r.pixels.is_cuda and r.pixels.dtype == torch.uint8
        assert r.pixels.shape == shape and np.array_equal(r.pixels.cpu().numpy(), np.asarray(Image.open(p)))
    host = read_masks(paths, dev, "host")
    assert [r.where for r in host] == ["host", "host"] and all(torch.equal(h.pixels, r.pixels) for h, r in zip(host, reads))


@pytest.mark.parametrize("rows", [None, 5])
def test_round_trip_with_the_device_encoder(dev, tmp_path, rows):
    from flair_amd import ops
    from flair_amd.tiff import read_masks
    from flair_amd.writer import tiff_lzw_file
    x = torch.from_numpy(np.stack([dc.small_image(64, 96, seed=1), dc.small_image(64, 96, k=256, seed=2)])).to(dev)
    slots, counts, _, R = ops.tiff_lzw_encode(x, rows_per_strip=rows)
    slots, counts = slots.cpu().numpy(), counts.cpu().numpy()
    paths = []
    for b in range(2):
        paths.append(tmp_path / f"tile{b}.tif")
        paths[-1].write_bytes(tiff_lzw_file(64, 96, R, [slots[b, s, :counts[b, s]].tobytes() for s in range(counts.shape[1])]))
    reads = read_masks(paths, dev, "device")
    assert [r.where for r in reads] == ["device"] * 2
    assert torch.equal(torch.stack([r.pixels for r in reads]), x)


def _bad_strips():
    """(name, stream, dst_len, mode, status) of the defined failures, with the reference decoder's own status"""
    C, E = (256, 9), (257, 9)
    s = dc.values_strip(4000, 19)
    enc = tc.lzw_strip(s)
    out = [("cut_in_half", enc[:len(enc) // 2], len(s), 1, 1),
           ("clear_eoi", dc.pack_codes([C, E]), 4, 1, 2),
           ("nonliteral_first", dc.pack_codes([C, (300, 9)]), 4, 1, 3),
           ("code_beyond_nxt", dc.pack_codes([C, (65, 9), (400, 9)]), 4, 1, 4),
           ("empty_stream", b"", 4, 1, 1),
           ("stored_short", bytes(10), 12, 0, 1)]
    rng = np.random.default_rng(77)
    for i in range(20):
        g = rng.integers(0, 256, int(rng.integers(64, 301))).astype(np.uint8).tobytes()
        want = int(rng.integers(1, 3000))
        out.append((f"random_{i}", g, want, 1, dc.lzw_decode_strip(g, want)[1]))
    for name, stream, want, mode, st in out:
        if mode == 1:
            assert dc.lzw_decode_strip(stream, want)[1] == st, name
    return out


def test_defined_failures(dev):
    bad = _bad_strips()
    good = [g for g in GOOD if g[0] in ("boundary_5999", "constant_16384", "cap_65536", "stored_37")]
    assert len(good) == 4
    # range and cap errors: dst_len 0, an LZW dst_len above the cap, and (last, with src_bytes cut by one) a stream past the source
    stream = tc.lzw_strip(b"abcabcabc")
    ranges = [("dst_len_0", stream, 0, 1), ("over_the_cap", stream, dc.MAX_STRIP + 1, 1), ("negative_len", stream, -3, 1),
              ("unknown_mode", stream, 9, 2)]
    strips = []
    for k, (_, enc, want, mode) in enumerate(good):
        strips += [(b[1], b[2], b[3]) for b in bad[k::4]] + [(enc, len(want), mode)]
    strips += [(r[1], r[2], r[3]) for r in ranges] + [(stream, 9, 1)]
    want_status = []
    for k in range(4):
        want_status += [b[4] for b in bad[k::4]] + [0]
    want_status += [5] * len(ranges) + [5]
    total = sum(len(s[0]) for s in strips)
    dst, status, dst_off, dst_len = _launch(dev, strips, misalign=5, src_bytes=total - 1)
    assert status.tolist() == want_status
    assert dc.guards_intact(dst, dst_off, dst_len)
    for (enc, want, mode), st, o in zip(strips, status, dst_off):
        region = dst[o:o + max(want, 0)]
        if st == 5:
            assert (region == dc.FILL).all()                         # nothing of such a strip is written
        elif mode == 1:
            ref, ref_st = dc.lzw_decode_strip(enc, want)
            assert ref_st == st and region[:len(ref)].tobytes() == ref and (region[len(ref):] == dc.FILL).all()
        elif st == 0:
            assert region.tobytes() == enc[:want]
    assert set(want_status) == {0, 1, 2, 3, 4, 5}


def _classes(C):
    return {k + 1: [1 if k != 4 else 0, f"class{k}"] for k in range(C)}


def _build_metrics_fixture(root):
    """8 pairs of 64 x 96, 13 classes, truth stored as class + 1: LZW truth by PIL, predictions alternately by PIL and by
    tiff_lzw_file; pair 1 a stored truth, 2 a deflate truth, 3 a prediction of another size, 4 a truncated prediction, 5 a
    prediction whose second strip holds a corrupted code"""
    from flair_amd.writer import tiff_lzw_file
    C, n, H, W = 13, 8, 64, 96
    (root / "gt").mkdir()
    preds_dir = root / "run" / "predictions"
    preds_dir.mkdir(parents=True)
    rows, names = [], {}
    for i in range(n):
        truth = dc.small_image(H, W, k=C + 2, seed=100 + i)          # 0 and C + 1 fall outside the classes
        pred = np.where(np.random.default_rng(200 + i).random((H, W)) < 0.2, dc.small_image(H, W, k=C, seed=300 + i),
                        np.clip(truth.astype(np.int64) - 1, 0, C - 1)).astype(np.uint8)
        t_path, p_path = root / "gt" / f"MSK_{i:06d}.tif", preds_dir / f"PRED_IMG_{i:06d}.tif"
        Image.fromarray(truth).save(t_path, **({} if i == 1 else {"compression": "tiff_adobe_deflate" if i == 2 else "tiff_lzw"}))
        if i == 3:
            Image.fromarray(pred[:, :80]).save(p_path, compression="tiff_lzw")
        elif i % 2 == 0:
            Image.fromarray(pred).save(p_path, compression="tiff_lzw")
        else:
            strips = tc.ref_strips(pred, 16)
            if i == 5:   # an 12-bit-wide hole of ones in the middle of strip 1: a code far beyond the table
                s = bytearray(strips[1])
                s[20:23] = b"\xff\xff\xff"
                strips[1] = bytes(s)
            p_path.write_bytes(tiff_lzw_file(H, W, 16, strips))
        if i == 4:
            p_path.write_bytes(p_path.read_bytes()[:200])
        rows.append(f"/data/x/img/IMG_{i:06d}.tif,{t_path}")
        names[i] = (t_path, p_path)
    (root / "test.csv").write_text("\n".join(rows) + "\n")
    return {"paths": {"test_csv": str(root / "test.csv")}, "classes": _classes(C)}, preds_dir, names


@pytest.fixture(scope="module")
def metrics_fixture(tmp_path_factory):
    return _build_metrics_fixture(tmp_path_factory.mktemp("metrics_decode"))


@pytest.fixture(scope="module")
def host_result(dev, metrics_fixture):
    return _run_metrics(dev, metrics_fixture, "host", 64)


def _run_metrics(dev, fixture, decode, chunk_tiles):
    import contextlib
    import io
    from flair_amd import metrics as M
    config, preds_dir, _ = fixture
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        out = M.metrics(config, preds_dir, device=dev, chunk_tiles=chunk_tiles, decode=decode)
    folder = preds_dir.parent / "metrics"
    errors = [line.split(":")[0] for line in printed.getvalue().splitlines() if line.startswith("Error at index")]
    return out, np.load(folder / "confmat.npy"), json.load(open(folder / "metrics.json")), errors, dict(M.metrics.last_read_stats)


def test_metrics_fixture_is_what_it_says(dev, metrics_fixture, host_result):
    from flair_amd.tiff import tiff_strip_layout
    _, _, names = metrics_fixture
    out, cm, saved, errors, stats = host_result
    assert errors == ["Error at index 3", "Error at index 4", "Error at index 5"]      # PIL itself refuses these three pairs
    assert stats == {"decode": "host", "device": 0, "host": 0, "host_after_device_error": 0, "error": 0}
    assert cm.sum() > 0 and cm.shape == (13, 13)
    assert tiff_strip_layout(names[2][0].read_bytes()) is None and tiff_strip_layout(names[1][0].read_bytes()).compression == 1
    assert tiff_strip_layout(names[5][1].read_bytes()) is not None      # the corrupted file looks fine from its IFD


@pytest.mark.parametrize("chunk_tiles", [3, 64])
def test_metrics_device_mode_equals_host_mode(dev, metrics_fixture, host_result, chunk_tiles):
    out_h, cm_h, saved_h, errors_h, _ = host_result
    out_d, cm_d, saved_d, errors_d, stats = _run_metrics(dev, metrics_fixture, "device", chunk_tiles)
    assert np.array_equal(cm_d, cm_h) and cm_d.dtype == cm_h.dtype
    assert saved_d == saved_h and list(saved_d) == list(saved_h)
    assert list(out_d) == list(out_h) and all(np.array_equal(out_d[k], out_h[k]) for k in out_h)
    assert errors_d == errors_h
    # the fallbacks: the deflate truth alone is PIL's from the start; only the truncated and the corrupted prediction may have gone
    # to PIL after a device error or ended as errors; every other file was decoded by the kernel
    assert stats["decode"] == "device" and stats["host"] == 1
    assert stats["host_after_device_error"] + stats["error"] == 2
    assert stats["device"] == 16 - 3


def test_argument_errors_launch_nothing(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    stream = tc.lzw_strip(b"abcabcabc")
    src, src_off, src_len, dst_off, dst_len, mode, dst_bytes = dc.strip_table([(stream, 9, 1)])
    t = [torch.from_numpy(a).to(dev) for a in (src, src_off, src_len, dst_off, dst_len, mode)]
    dst = torch.full((dst_bytes,), dc.FILL, dtype=torch.uint8, device=dev)
    status = torch.full((1,), -7, dtype=torch.int32, device=dev)
    p = [L.ptr(x) for x in t]
    good = [p[0], src.size, p[1], p[2], p[3], p[4], p[5], 1, L.ptr(dst), dst_bytes, L.ptr(status), L.stream()]
    for at in (0, 2, 3, 4, 5, 6, 8, 10):          # every pointer in turn
        args = list(good)
        args[at] = None
        assert lib.flair_tiff_lzw_decode(*args) < 0
    for at, value in ((7, 0), (7, -1), (1, -1), (9, -1)):   # nstrips, src_bytes, dst_bytes
        args = list(good)
        args[at] = value
        assert lib.flair_tiff_lzw_decode(*args) < 0
    torch.cuda.synchronize()
    assert (dst.cpu() == dc.FILL).all() and (status.cpu() == -7).all()
    assert lib.flair_tiff_lzw_decode(*good) == 0
    assert status.cpu().tolist() == [0] and dst.cpu().numpy()[dst_off[0]:dst_off[0] + 9].tobytes() == b"abcabcabc"
    assert lib.flair_tiff_lzw_decode_max_strip() == dc.MAX_STRIP


def test_ops_wrapper(dev):
    from flair_amd import ops
    s = dc.values_strip(3000, 19)
    src, src_off, src_len, dst_off, dst_len, mode, dst_bytes = dc.strip_table([(tc.lzw_strip(s), 3000, 1), (s[:100], 100, 0)], guard=0)
    t = [torch.from_numpy(a).to(dev) for a in (src, src_off, src_len, dst_off, dst_len, mode)]
    out, status = ops.tiff_lzw_decode(*t, dst_bytes)
    assert out.dtype == torch.uint8 and out.shape == (3100,) and status.dtype == torch.int32 and status.tolist() == [0, 0]
    assert out.cpu().numpy().tobytes() == s + s[:100]
    with pytest.raises(ValueError):
        ops.tiff_lzw_decode(*t, 0)
