#!/usr/bin/env python3
"""Makes raylog_dxdy_16x16.json: the 16 x 16 direction map (include/isx.h, isx_exit_maps: bins over the direction cosines dx, dy)
of the exit directions the reference logged in its committed 3dRayLog.txt ("# dx dy dz", 100 000 lines).

usage: make_raylog_dxdy.py <path to the reference's 3dRayLog.txt>
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from exitmap_np import direction_map  # noqa: E402

N = 16


def main(path):
    d = np.loadtxt(path, comments="#")
    assert d.ndim == 2 and d.shape[1] == 3
    m, binned, outside = direction_map(d, N, N)
    out = {"source": "3dRayLog.txt", "n": int(d.shape[0]), "n_u": N, "n_v": N, "binned": binned, "outside": outside,
           "dir_map": m.astype(int).tolist()}
    with open(os.path.join(HERE, "raylog_dxdy_16x16.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(out["n"], binned, outside, int((m > 0).sum()))


if __name__ == "__main__":
    main(sys.argv[1])
