"""Fixed inputs of the host framers (writer.tiff_lzw_file, raster_writer.tiled_tiff_header / tiled_tiff_ifd) whose output bytes are
recorded in tests/golden/tiff_framing.json (tests/golden/make_golden_tiff_framing.py), and the call that frames one of them."""
import raster_writer_cases as wc

H, W, TILE = 37, 53, 16          # the odd raster: 3 x 4 tiles


def _payload(i, n):
    """n bytes that stand for a compressed stream (the framers do not look inside)"""
    return bytes((7 * i + 3 * j) % 251 for j in range(n))


def framing_inputs():
    """name -> (function name, keyword arguments)"""
    cases = {}
    for n in (1, 4):
        strips = [_payload(i, 20 + 13 * i) for i in range(n)]
        cases[f"lzw_file_{n}_strips"] = ("tiff_lzw_file", dict(H=64, W=96, rows_per_strip=64 // n, strips=strips))
    for name, off, big in (("classic_8", 8, False), ("classic_far", (1 << 32) - 2, False), ("big_16", 16, True), ("big_far", (1 << 40) + 6, True)):
        cases[f"header_{name}"] = ("tiled_tiff_header", dict(ifd_offset=off, bigtiff=big))
    geo = wc.geo_source()[1]
    for bands in (1, 2, 3, 13):
        for il in ("band", "pixel"):
            n = (bands if il == "band" else 1) * -(-H // TILE) * -(-W // TILE)
            counts = [50 + (37 * i) % 211 for i in range(n)]
            offsets, at = [], 16
            for c in counts:
                offsets.append(at)
                at += -(-c // 16) * 16
            for big in (False, True):
                for tags in (None, geo):
                    name = f"ifd_b{bands}_{il}_{'big' if big else 'classic'}{'_geo' if tags else ''}"
                    cases[name] = ("tiled_tiff_ifd", dict(H=H, W=W, bands=bands, tile=TILE, interleave=il, offsets=offsets, counts=counts,
                                                          ifd_offset=at, bigtiff=big, geo_tags=tags))
    return cases


def frame(function, kwargs) -> bytes:
    from flair_amd import raster_writer, writer
    f = getattr(writer, function, None) or getattr(raster_writer, function)
    return f(**kwargs)
