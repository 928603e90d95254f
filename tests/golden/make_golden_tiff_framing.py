#!/usr/bin/env python3
"""Generate tests/golden/tiff_framing.json: the bytes ``writer.tiff_lzw_file``, ``raster_writer.tiled_tiff_header`` and
``raster_writer.tiled_tiff_ifd`` produced for the fixed inputs of tests/tiff_framing_cases.py at the commit BEFORE the framers were
expressed through ``flair_amd/tiff_ifd.py`` (80eeff9, "zone_detect: read the input raster from a tiled LZW TIFF on the GPU").

    git checkout 80eeff9 -- flair-1_amd/flair_amd && python tests/golden/make_golden_tiff_framing.py

The file records what the hand-written framers of that commit laid out (entry order, inline values, where the out-of-line arrays lie
and how they are padded), so that tests/test_tiff_ifd_cpu.py can hold every later framer to the same bytes.  Run it again only to
add inputs, and then from that commit: run from a later one it records nothing but the code under test.

Output is DATA only: {name: hex of the framed bytes}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "flair-1_amd")):
    sys.path.insert(0, p)

import tiff_framing_cases as fc   # noqa: E402


def main():
    out = {name: fc.frame(function, kwargs).hex() for name, (function, kwargs) in fc.framing_inputs().items()}
    with open(os.path.join(HERE, "tiff_framing.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote tiff_framing.json:", len(out), "cases,", sum(len(v) // 2 for v in out.values()), "bytes framed")


if __name__ == "__main__":
    main()
