"""Records the moment tests (tests/moments.py) in profiles/moments_measure.json.

--part gpu (one GPU): for every case of tests/test_gpu_moments.py the
realisations used, the largest z per family (a, b, c, off, d) with its index,
and the seconds spent in setup (engine, dsce_build_mmse, dsce_get_correlation,
dsce_get_W), in dsce_export and in the host's accumulation; then the negative
control (the default case's samples against the analytic side at 515 km/h).

--part host (no GPU): the same for the oracle's realisations of
tests/test_moments_host.py, the scan of the fD factor around the smallest one
caught, and the other negative controls.

The cases, seeds and n are the tests'.  Each part replaces its own section of
the file and leaves the other.

    python tools/moments_measure.py --part host --out profiles/moments_measure.json
    python tools/moments_measure.py --part gpu --out profiles/moments_measure.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "channel-estimation_amd"), ROOT]


def gpu_part():
    import torch      # before the engine's library: one HIP runtime for both

    import harness
    import test_gpu_moments as t
    res = {"device": torch.cuda.get_device_name(0), "seed": t.SEED, "snr_db": list(t.SNR), "chunk": t.CHUNK,
           "asserted": {"ofdm": ["a", "b", "c", "off", "d"], "fbmc_aux": ["a", "b", "c"], "fbmc_cod": ["a", "b", "c"]},
           "cases": [], "controls": []}
    t.measure("default", n=t.CHUNK)                                  # warm-up: library load, first launches
    for case in t.CASES:
        t0 = time.perf_counter()
        r = t.measure(case)
        r["seconds"]["total"] = round(time.perf_counter() - t0, 3)
        res["cases"].append(r)
    wrong = ("ofdm", harness.setup("default", schemes=("ofdm",), snr_db=t.SNR, velocity_kmh=515.0))
    r = t.measure("default", setup=wrong)
    r["control"] = "analytic side at 515 km/h (fD x 1.03)"
    res["controls"].append(r)
    return res


def host_part():
    import numpy as np

    import test_moments_host as t
    res = {"seed": t.SEED, "snr_db": list(t.SNR), "fd_caught": t.FD_CAUGHT, "cases": [], "fd_scan": [], "controls": []}
    for gid, n in (t.MAIN,) + t.SMALL:
        t0 = time.perf_counter()
        z = t.check_null(gid, n)
        T = t.setup_of(gid)[0]
        res["cases"].append(dict(case=gid, n=n, z={f: round(v[0], 3) for f, v in z.items()},
                                 asserted=["a", "b", "c"] + (["off", "d"] if T.kind == "ofdm" else []),
                                 seconds=round(time.perf_counter() - t0, 3)))
    T, S, sc, M, fam, h, hp = t.sampled(*t.MAIN)
    for f in (0.90, 0.92, 0.93, 0.94, 0.96, 1.04, 1.06, 1.07, 1.08, 1.10, 1.5, 2 * np.pi):
        z = t._scores(fam, S, sc, fd_scale=f)
        res["fd_scan"].append(dict(factor=round(float(f), 4), z={k: round(v[0], 3) for k, v in z.items() if k != "d"}))
    pn = np.asarray(S.chan["pdp_norm"], dtype=float)
    taps = np.flatnonzero(pn)
    swapped = pn.copy()
    swapped[[taps[0], taps[-1]]] = swapped[[taps[-1], taps[0]]]
    for name, mut in (("Uniform for Jakes", dict(model="Uniform")), ("first and last PDP tap swapped", dict(pdp_norm=swapped)),
                      ("pn x 1.5", dict(pn_scale=1.5)), ("kappa x 2", dict(kappa_scale=2.0))):
        z = t._scores(fam, S, sc, **mut)
        res["controls"].append(dict(control=name, case=t.MAIN[0], n=t.MAIN[1],
                                    z={k: round(v[0], 3) for k, v in z.items() if k != "d"}))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--part", choices=("gpu", "host"), required=True)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    import moments
    res = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res["bar"] = moments.BAR
    res[a.part] = gpu_part() if a.part == "gpu" else host_part()
    txt = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
