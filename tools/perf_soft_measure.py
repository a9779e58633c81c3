"""Measures the soft kernels with DSCE_LLR_PERFECT against the unflagged ones on
one GPU at the C2 export shape of DESIGN.md section 7g (default config, OFDM, 7 SNR
points, n_iter 4, 8192 realisations at batch 8192):

  * kernel time (dsce_kernel_time) of k_llr (only llr, float32, device
    destination), k_llr_info (loss_est alone: the S stages of either branch) and
    k_llr_calib (ratio_est alone), exact LLRs, flagged and unflagged in the same
    process, after a warm-up call, alternating, `repeats` calls each;
  * the end-to-end figures of DESIGN.md section 7j: rho of both branches from
    realisations 5..68, and the exact-LLR rate on realisations 69..132, raw and
    with pn_eff <- rho pn_eff, at 35 dB.

    python tools/perf_soft_measure.py --out profiles/perf_soft_measure.json
"""
import argparse
import json
import os
import sys

import torch          # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "channel-estimation_amd")]

import numpy as np    # noqa: E402

SEED = 0x5EED0002
E2E_SEED = 0x5EED0009
BRANCHES = ("mmse", "perfect")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=a.batch)
    res = {"config": "default", "scheme": "ofdm", "n_snr": len(S.snr_db), "n_iter": int(S.n_iter), "reps": a.reps,
           "batch": a.batch, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "kernel_ms": {},
           "launches": {}}

    def timed(name, fn):
        """fn() with timing on: (kernel `name` ms, launches) of that call alone."""
        eng.enable_timing(True)
        n0, t0 = eng.kernel_time(name)
        fn()
        n1, t1 = eng.kernel_time(name)
        eng.enable_timing(False)
        return t1 - t0, n1 - n0

    calls = {
        "k_llr": lambda br: eng.export_llr_torch(0, SEED, 0, a.reps, fields=("llr",), dtype=torch.complex64, branch=br),
        "k_llr_info": lambda br: eng.run_soft(0, SEED, 0, a.reps, "exact",
                                              {"loss_est": np.zeros(eng.soft_shapes(0)["loss_est"])}, branch=br),
        "k_llr_calib": lambda br: eng.run_calib(0, SEED, 0, a.reps,
                                                {"ratio_est": np.zeros(eng.calib_shapes(0)["ratio_est"])}, branch=br),
    }
    for kernel, call in calls.items():                      # warm-up (buffers, clocks, code objects)
        for br in BRANCHES:
            call(br)
    for kernel, call in calls.items():
        ms = {br: [] for br in BRANCHES}
        for _ in range(a.repeats):                           # alternating
            for br in BRANCHES:
                t, n = timed(kernel, lambda: call(br))
                ms[br].append(t)
                res["launches"][kernel] = n
        res["kernel_ms"][kernel] = ms
    torch.cuda.empty_cache()

    # rho from realisations 5..68, the rate on 69..132 (as DESIGN.md 7i), 35 dB, all symbols
    eng.set_batch(64)
    k = int(np.argmin(np.abs(np.asarray(S.snr_db) - 35.0)))
    e2e = {"seed": E2E_SEED, "snr_db": float(S.snr_db[k]), "rho_reps": [5, 68], "rate_reps": [69, 132]}
    for br in BRANCHES:
        rho = eng.run_calib(0, E2E_SEED, 5, 64, branch=br)["ratio_est"] / 64
        raw = eng.bicm_rate(0, eng.run_soft(0, E2E_SEED, 69, 64, branch=br)["loss_est"], 64)
        if br == "mmse":
            eng.set_llr_scale(0, rho)
        else:
            eng.set_llr_scale_perf(0, rho)
        cal = eng.bicm_rate(0, eng.run_soft(0, E2E_SEED, 69, 64, branch=br)["loss_est"], 64)
        e2e[br] = {"rho_mean": rho.mean(axis=-1)[k].tolist(), "rate_raw": raw[k, :, 0].tolist(),
                   "rate_calibrated": cal[k, :, 0].tolist()}
    eng.set_llr_scale(0)
    eng.set_llr_scale_perf(0)
    res["e2e"] = e2e
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
