"""Measures dsce_run_calib (k_llr_calib) on one GPU at the C2 export shape of
DESIGN.md sections 7g / 7h (default config, OFDM, 7 SNR points, n_iter 4, 8192
realisations at batch 8192), beside dsce_run_soft's kernel in the same process:

  * kernel time (dsce_kernel_time) of k_llr_calib with both outputs, of
    k_llr_info max-log with both outputs, and of k_llr_info exact without
    tables, with tables of ones (the same LLRs, so the same data-dependent
    branches: what the scale load itself costs) and with rho of a calibration
    call installed (other LLRs), after one warm-up call each, alternating,
    `repeats` calls each;
  * wall time of run_calib.

    python tools/calib_measure.py --out profiles/calib_measure.json
"""
import argparse
import json
import os
import sys
import time

import torch          # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "channel-estimation_amd")]

SEED = 0x5EED0002


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
           "batch": a.batch, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "kernel_ms": {}, "wall_s": {}}

    def timed(name, fn):
        """fn() with timing on: (kernel `name` ms, launches, wall s, result) of that call alone."""
        eng.enable_timing(True)
        n0, t0 = eng.kernel_time(name)
        w0 = time.perf_counter()
        out = fn()
        w = time.perf_counter() - w0
        n1, t1 = eng.kernel_time(name)
        eng.enable_timing(False)
        return t1 - t0, n1 - n0, w, out

    calib = lambda: eng.run_calib(0, SEED, 0, a.reps)
    soft = lambda method: eng.run_soft(0, SEED, 0, a.reps, method)
    rho = calib()                                            # warm-up (buffers, clocks, code objects), and the tables
    rho = {f: v / a.reps for f, v in rho.items()}
    for method in ("exact", "maxlog"):
        soft(method)
    ones = {f: v * 0 + 1 for f, v in rho.items()}
    kc, wc, km, ke, k1, ks = [], [], [], [], [], []
    for _ in range(a.repeats):                               # alternating
        t, n, w, _ = timed("k_llr_calib", calib)
        kc.append(t)
        wc.append(w)
        res["launches_k_llr_calib"] = n
        km.append(timed("k_llr_info", lambda: soft("maxlog"))[0])
        t, n, w, raw = timed("k_llr_info", lambda: soft("exact"))
        ke.append(t)
        res["launches_k_llr_info"] = n
        eng.set_llr_scale(0, ones["ratio_est"], ones["ratio_perf0"])
        k1.append(timed("k_llr_info", lambda: soft("exact"))[0])
        eng.set_llr_scale(0, rho["ratio_est"], rho["ratio_perf0"])
        t, n, w, cal = timed("k_llr_info", lambda: soft("exact"))
        ks.append(t)
        eng.set_llr_scale(0)
    res["kernel_ms"] = {"k_llr_calib": kc, "k_llr_info_maxlog": km, "k_llr_info_exact": ke,
                        "k_llr_info_exact_scaled_by_ones": k1,
                        "k_llr_info_exact_scaled": ks}
    res["wall_s"]["run_calib"] = wc
    res["rho_mean_last_snr"] = rho["ratio_est"][-1].mean(axis=-1).tolist()
    res["rate_exact_last_snr_all"] = eng.bicm_rate(0, raw["loss_est"], a.reps)[-1, :, 0].tolist()
    res["rate_exact_last_snr_all_calibrated_in_sample"] = eng.bicm_rate(0, cal["loss_est"], a.reps)[-1, :, 0].tolist()
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
