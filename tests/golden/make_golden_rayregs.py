"""Writes tests/golden/rayregs.npz: the seeded synthetic cases of the distortion loss (tests/raydist64.py) at the small shapes, their float64
results (direct double sum over explicit midpoints, autograd), and the measured fp32 floors of the same program on every case, on an
S = 1024 case and on the two real weight maps of hotpath.npz.  Data only; the reference has no distortion term, so nothing of it is used.

    python tests/golden/make_golden_rayregs.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import raydist64 as r64     # noqa: E402


def main():
    gold = np.load(os.path.join(HERE, "hotpath.npz"))
    out = {}
    for case in r64.CASES:
        for (R, S) in r64.SMALL:
            seed = r64.CASES.index(case) * 100 + S
            w = r64.named_case(case, R, S, seed)
            t_min, u, step = r64.geometry(R, S, seed)
            y = r64.distortion(w, t_min, step, u)
            key = f"{case}:{R}x{S}"
            out[key + ":w"], out[key + ":t_min"], out[key + ":u"], out[key + ":step"] = w, t_min, u, np.float64(step)
            out[key + ":loss"], out[key + ":grad"], out[key + ":per_ray"] = np.float64(y["loss"]), y["grad"], y["per_ray"]
    for k, v in r64.measure_floors(gold).items():
        out["ref32_err:" + k] = np.float64(v)
        print("ref32_err", k, v)
    path = os.path.join(HERE, "rayregs.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
