"""How often the host rejects the reciprocal division near a family J target (host-only, no GPU).

Asks sbmp_division_reciprocal for R1Size = W / 16 of `--count` consecutive float32 widths centred
on the `up` width of the first x-odd round-up triple at the small site (tests/region_scenarios.py;
R2Size for n = 8 has the same mantissa) and prints how many the host rejected.  About 40 ms per
divisor and thread: 65,536 widths take some 9 minutes on 8 threads.  DESIGN.md section 3 (family J)
quotes the result.

    python tools/scan_division_reciprocal.py [--count 65536] [--threads 8]
"""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 16)
    ap.add_argument("--threads", type=int, default=8)
    a = ap.parse_args()
    import region_scenarios as R
    from cudasbmp_amd.kgmt import division_reciprocal
    t = R.r1_triples(R.SMALL, "car", 0, R.R1_SEARCHES[0][2])[0]
    widths = R.ulps(np.full(a.count, t.up, dtype=np.float32), np.arange(a.count) - a.count // 2)
    t0 = time.time()
    with ThreadPoolExecutor(a.threads) as ex:   # the call releases the GIL
        y = list(ex.map(lambda w: division_reciprocal(float(np.float32(w) / np.float32(16))), widths))
    rejected = [float(w) for w, r in zip(widths, y) if r == 0.0]
    print(f"target width {t.up!r} (slot {t.slot}, line {t.c}); widths {float(widths[0])!r} .. {float(widths[-1])!r}; "
          f"{len(rejected)} of {a.count} rejected {rejected[:8]}; {time.time() - t0:.0f} s")


if __name__ == "__main__":
    main()
