"""tiff_chunks_to_batch_kernel (csrc/tiff_read.hip) through the C ABI, and tile_loader.read_tiles / TileLoader on top of it: one
launch over a table that reaches every branch against the numpy restatement, batches of files of mixed layouts against their
pixels and against read_raster, the loader's batches against oracle.data_feed, prefetched batches that must stay intact, and the
defined failure of a truncated chunk.  Byte and integer work, and TileFeed's arithmetic that is pinned bit-exact: every assertion is
exact."""
import numpy as np
import pytest
import torch

import raster_reader_cases as rc
import tile_loader_cases as lc
from flair_amd import raster_reader as rr
from flair_amd import tile_loader as tl

pytestmark = pytest.mark.gpu

MEANS = [105.08, 110.87, 101.82, 106.38, 53.26]
STDS = [52.17, 45.38, 44, 39.69, 79.3]


def test_chunks_to_batch_through_the_c_abi(dev):
    from flair_amd import _lib as L
    lib = L.lib()
    scratch, table, status, max_rows = lc.kernel_launch()
    want = lc.batch_ref(list(scratch), table, status, np.full(lc.KERNEL_SHAPE, lc.FILL, np.uint8), lc.KERNEL_SLOT)
    P, H, W = lc.KERNEL_SHAPE
    d_scratch, d_table, d_status = (torch.from_numpy(a).to(dev) for a in (scratch, table, status))
    # a guard plane before and after: nothing outside the planes is written either
    buf = torch.full((P + 2, H, W), lc.FILL, dtype=torch.uint8, device=dev)
    planes = buf[1:P + 1]
    n = len(table)
    call = lambda s, t, st, nn, rows, p, np_, h, w: lib.flair_tiff_chunks_to_batch(s, lc.KERNEL_SLOT, t, st, nn, rows, p, np_, h, w,  # noqa: E731
                                                                                   L.stream())
    ptrs = (L.ptr(d_scratch), L.ptr(d_table), L.ptr(d_status))
    assert call(*ptrs, n, max_rows, L.ptr(planes), P, H, W) == 0
    got = buf.cpu().numpy()
    assert np.array_equal(got[1:P + 1], want)                       # every written byte, and every byte that must still be the fill
    assert (got[0] == lc.FILL).all() and (got[-1] == lc.FILL).all()
    # the launch is sized by max_rows only: a smaller grid walks the same rows
    again = torch.full((P, H, W), lc.FILL, dtype=torch.uint8, device=dev)
    assert call(*ptrs, n, 1, L.ptr(again), P, H, W) == 0 and np.array_equal(again.cpu().numpy(), want)
    # return codes
    for bad in ((None, ptrs[1], ptrs[2]), (ptrs[0], None, ptrs[2]), (ptrs[0], ptrs[1], None)):
        assert call(*bad, n, max_rows, L.ptr(again), P, H, W) == -1
    assert call(*ptrs, n, max_rows, None, P, H, W) == -1
    for nn, rows, np_, h, w in ((0, max_rows, P, H, W), (n, 0, P, H, W), (n, max_rows, 0, H, W), (n, max_rows, P, 0, W), (n, max_rows, P, H, 0)):
        assert call(*ptrs, nn, rows, L.ptr(again), np_, h, w) == -1
    assert lib.flair_tiff_chunks_to_batch(ptrs[0], 0, ptrs[1], ptrs[2], n, max_rows, L.ptr(again), P, H, W, L.stream()) == -1
    odd = torch.zeros(8 * n * 4 + 4, dtype=torch.uint8, device=dev)
    assert call(ptrs[0], L.ptr(odd[2:]), ptrs[2], n, max_rows, L.ptr(again), P, H, W) == -2
    assert call(ptrs[0], ptrs[1], L.ptr(odd[1:]), n, max_rows, L.ptr(again), P, H, W) == -2
    torch.cuda.synchronize()
    assert np.array_equal(again.cpu().numpy(), want)               # the refused calls wrote nothing


def test_ops_wrapper_takes_batches_and_refuses_other_shapes(dev):
    from flair_amd import _lib as L
    from flair_amd import ops
    scratch, table, status, _ = lc.kernel_launch()
    want = lc.batch_ref(list(scratch), table, status, np.full(lc.KERNEL_SHAPE, lc.FILL, np.uint8), lc.KERNEL_SLOT)
    d_scratch, d_table, d_status = (torch.from_numpy(a).to(dev) for a in (scratch, table, status))
    planes = torch.full((3, 3, 37, 130), lc.FILL, dtype=torch.uint8, device=dev)      # (B, bands, H, W): nine planes
    assert ops.tiff_chunks_to_batch(d_scratch, d_table, d_status, planes) is planes
    assert np.array_equal(planes.cpu().numpy().reshape(lc.KERNEL_SHAPE), want)
    with pytest.raises(L.FlairHipError):
        ops.tiff_chunks_to_batch(d_scratch, d_table[:, :5].contiguous(), d_status, planes)
    with pytest.raises(L.FlairHipError):
        ops.tiff_chunks_to_batch(d_scratch, d_table, d_status, planes.float())


def _check_read(dev, tmp_path, n, group_bytes=None):
    ip, img, mp, msk = lc.write_set(tmp_path, n)
    kw = {} if group_bytes is None else {"group_bytes": group_bytes}
    got_img, got_msk = tl.read_tiles(ip, mp, dev, **kw)
    assert got_img.dtype == got_msk.dtype == torch.uint8 and got_img.is_contiguous() and got_msk.is_contiguous()
    assert tuple(got_img.shape) == (n, 5, 32, 32) and tuple(got_msk.shape) == (n, 32, 32) and got_img.device == got_msk.device == dev
    assert np.array_equal(got_img.cpu().numpy(), img) and np.array_equal(got_msk.cpu().numpy(), msk)
    return ip, got_img


def test_read_tiles_of_mixed_layouts(dev, tmp_path):
    ip, got = _check_read(dev, tmp_path, 5)
    assert torch.equal(got, torch.stack([rr.read_raster(p, dev) for p in ip]))
    only, none = tl.read_tiles(ip, None, dev)
    assert none is None and torch.equal(only, got)
    ip, small = _check_read(dev, tmp_path, 5, group_bytes=4096)
    assert torch.equal(small, got)
    plan = tl.plan_batch([open(p, "rb").read() for p in ip], 4096)
    assert len(plan.groups) > 1 and plan.slot == 5120                   # one_strip makes the slot larger than the group: one chunk each


def _draws():
    return [(v, h, k) for v in (0, 1) for h in (0, 1) for k in range(4)]


def test_loader_against_the_oracle(dev, tmp_path):
    from flair_amd.data_feed import TileFeed, pack_d4
    from oracle import data_feed as F
    B = 16
    ip, img, mp, msk = lc.write_set(tmp_path, B)
    draws = _draws()
    d4 = torch.tensor([pack_d4(*d) for d in draws], dtype=torch.uint8)
    mtd = np.random.default_rng(3).random((B, 45))
    files = {"IMG": ip, "MSK": mp, "MTD": mtd.tolist()}
    for channels in ([1, 2, 3, 4, 5], [3, 1, 5]):
        sel = [c - 1 for c in channels]
        for mode in ("custom", "scaling", "without"):
            feed = TileFeed(channels, 19, mode, MEANS, STDS)
            with_draws = lambda i, m, mtd=None, ids=None: feed(i, m, d4=d4, mtd=mtd, ids=ids)   # noqa: E731
            batches = list(tl.TileLoader(files, with_draws, batch_size=B, device=dev))
            assert len(batches) == 1 and sorted(batches[0]) == ["img", "msk", "mtd"]
            b = batches[0]
            assert b["img"].dtype == torch.float32 and tuple(b["img"].shape) == (B, len(channels), 32, 32) and b["msk"].dtype == torch.uint8
            got_img, got_msk = b["img"].cpu().numpy(), b["msk"].cpu().numpy()
            for s, (v, h, k) in enumerate(draws):
                assert np.array_equal(got_img[s], F.norm_np(F.d4_np(img[s][sel], v, h, k), mode, MEANS, STDS)), (channels, mode, v, h, k)
                assert np.array_equal(got_msk[s], F.d4_np(F.labels_from_raw(msk[s], 19), v, h, k)), (channels, mode, v, h, k)
            assert b["mtd"].dtype == torch.float32 and b["mtd"].device == dev
            assert torch.equal(b["mtd"].cpu(), torch.as_tensor(mtd, dtype=torch.float32))
    assert msk.min() == 0 and msk.max() == 24


def test_loader_non_square_predict_and_metadata(dev, tmp_path):
    from flair_amd.data_feed import TileFeed
    from oracle import data_feed as F
    n, H, W = 5, 40, 56
    ip, img, mp, msk = [], [], [], []
    for i in range(n):
        (data, raster), (mdata, raw) = lc.image_file(i, H, W), lc.mask_file(i, H, W)
        ip.append(str(tmp_path / f"IMG_{i}.tif")), mp.append(str(tmp_path / f"MSK_{i}.tif"))
        (tmp_path / f"IMG_{i}.tif").write_bytes(data), (tmp_path / f"MSK_{i}.tif").write_bytes(mdata)
        img.append(raster), msk.append(raw)
    mtd = np.random.default_rng(4).random((n, 45))
    feed = TileFeed([1, 2, 3, 4, 5], 13, "scaling")
    fit = list(tl.TileLoader({"IMG": ip, "MSK": mp}, feed, batch_size=3, device=dev))
    assert [b["img"].shape[0] for b in fit] == [3, 2] and all(sorted(b) == ["img", "msk"] for b in fit)
    got_img, got_msk = torch.cat([b["img"] for b in fit]).cpu().numpy(), torch.cat([b["msk"] for b in fit]).cpu().numpy()
    for s in range(n):
        assert np.array_equal(got_img[s], F.norm_np(img[s], "scaling")) and np.array_equal(got_msk[s], F.labels_from_raw(msk[s], 13))
    # predict: no masks, one tile a batch, the paths as ids, the metadata rows in file order
    config = {"batch_size": 4, "channels": [1, 2, 3, 4, 5], "classes": {i + 1: [1, str(i)] for i in range(13)}, "norm_type": "without",
              "norm_means": [], "norm_stds": [], "use_augmentation": True, "use_metadata": True}
    pred = list(tl.TileLoader.from_config(config, {"IMG": ip, "MSK": mp, "MTD": mtd.tolist()}, "predict", device=dev))
    assert len(pred) == n
    for s, b in enumerate(pred):
        assert sorted(b) == ["id", "img", "mtd"] and b["id"] == [ip[s]]
        assert np.array_equal(b["img"][0].cpu().numpy(), img[s].astype(np.float32))
        assert torch.equal(b["mtd"].cpu(), torch.as_tensor(mtd[s:s + 1], dtype=torch.float32))


def test_prefetched_batches_stay_intact(dev, tmp_path):
    from flair_amd.data_feed import TileFeed
    n = 14
    ip, img, mp, msk = lc.write_set(tmp_path, n)
    raw_feed = lambda i, m, mtd=None, ids=None: {"img": i, "msk": m}   # noqa: E731 - the bytes as read_tiles made them
    loader = tl.TileLoader({"IMG": ip, "MSK": mp}, raw_feed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5), device=dev)
    assert len(loader) == 4
    for epoch in range(2):
        order = tl.epoch_batches(n, 4, True, False, torch.Generator().manual_seed(5))
        if epoch == 1:       # the loader's generator has moved on: replay its second draw
            g = torch.Generator().manual_seed(5)
            tl.epoch_batches(n, 4, True, False, g)
            order = tl.epoch_batches(n, 4, True, False, g)
        batches = list(loader)                      # all four first: batch 0 has seen batches 1, 2 and 3 produced after it
        torch.cuda.synchronize()
        assert [b["img"].shape[0] for b in batches] == [4, 4, 4, 2]
        assert len({b["img"].data_ptr() for b in batches}) == 4 and len({b["msk"].data_ptr() for b in batches}) == 4
        for b, idx in zip(batches, order):
            assert np.array_equal(b["img"].cpu().numpy(), img[idx]) and np.array_equal(b["msk"].cpu().numpy(), msk[idx]), (epoch, idx)
    fed = list(tl.TileLoader({"IMG": ip, "MSK": mp}, TileFeed([1, 2, 3, 4, 5], 19, "without"), batch_size=4, device=dev))
    assert torch.equal(torch.cat([b["img"] for b in fed]).cpu(), torch.from_numpy(img).float())


def test_a_truncated_chunk_is_named_and_the_next_batch_is_unaffected(dev, tmp_path):
    ip, img, mp, msk = lc.write_set(tmp_path, 4)
    cut = lambda i, s: s[:len(s) // 2] if i == 7 else s   # noqa: E731 - the bytes run out: status 1, a defined outcome of the decoder
    bad = tmp_path / "IMG_cut.tif"
    bad.write_bytes(lc.image_file(0, mangle=cut)[0])       # tiled, band-interleaved: chunk 7 is the tile at (16, 16) of band 1
    with pytest.raises(rr.RasterDecodeError, match=r"chunk 7 \(tile at row 16, column 16, band 1\).*status 1") as e:
        tl.read_tiles([ip[1], str(bad), ip[2]], [mp[1], mp[0], mp[2]], dev)
    assert str(bad) in str(e.value) and (e.value.chunk, e.value.status) == (7, 1)
    got_img, got_msk = tl.read_tiles(ip, mp, dev)
    assert np.array_equal(got_img.cpu().numpy(), img) and np.array_equal(got_msk.cpu().numpy(), msk)
    with pytest.raises(rr.UnsupportedRaster, match="Compression"):
        (tmp_path / "deflate.tif").write_bytes(rc.refused_files()["deflate"][0])
        tl.read_tiles([ip[0], str(tmp_path / "deflate.tif")], None, dev)
