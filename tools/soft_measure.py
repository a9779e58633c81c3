"""Measures dsce_run_soft (k_llr_info) on one GPU at the C2 export shape of
DESIGN.md section 7g (default config, OFDM, 7 SNR points, n_iter 4, 8192
realisations at batch 8192), beside the way to the same sums it replaces:

  * kernel time (dsce_kernel_time) of k_llr_info, exact and max-log, with both
    outputs (S + 1 stages: the perfect-CSI one-tap receiver is one more) and
    with loss_est alone (the S stages k_llr demaps), and of k_llr with only llr
    requested (float32, device destination), same process, after a warm-up
    call, alternating, `repeats` calls each;
  * wall time of run_soft beside export_llr to the host (float32) plus the NumPy
    reduction dsce.modulation.bicm_info_loss, and how far the two results differ.

    python tools/soft_measure.py --out profiles/soft_measure.json
"""
import argparse
import json
import os
import sys
import time

import torch          # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "channel-estimation_amd")]

import numpy as np    # noqa: E402

SEED = 0x5EED0002


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--host-repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    from dsce.modulation import bicm_info_loss
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=a.batch)
    m = eng.llr_info(0)["m"]
    cons = np.asarray(S.schemes["ofdm"].considered_symbols).astype(bool)
    res = {"config": "default", "scheme": "ofdm", "n_snr": len(S.snr_db), "n_iter": int(S.n_iter), "reps": a.reps,
           "batch": a.batch, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "kernel_ms": {}, "wall_s": {}}

    def timed(name, fn):
        """fn() with timing on: (kernel `name` ms, launches, wall s) of that call alone."""
        eng.enable_timing(True)
        n0, t0 = eng.kernel_time(name)
        w0 = time.perf_counter()
        out = fn()
        w = time.perf_counter() - w0
        n1, t1 = eng.kernel_time(name)
        eng.enable_timing(False)
        return t1 - t0, n1 - n0, w, out

    soft = lambda method: eng.run_soft(0, SEED, 0, a.reps, method)
    est = lambda method: eng.run_soft(0, SEED, 0, a.reps, method, {"loss_est": np.zeros(eng.soft_shapes(0)["loss_est"])})
    dev = lambda method: eng.export_llr_torch(0, SEED, 0, a.reps, fields=("llr",), method=method, dtype=torch.complex64)
    for method in ("exact", "maxlog"):                       # warm-up (buffers, clocks, code objects)
        soft(method)
        dev(method)
    for method in ("exact", "maxlog"):
        ki, ke, kl, wi = [], [], [], []
        for _ in range(a.repeats):                           # alternating
            t, n, w, out = timed("k_llr_info", lambda: soft(method))
            ki.append(t)
            wi.append(w)
            res["launches_k_llr_info"] = n
            ke.append(timed("k_llr_info", lambda: est(method))[0])
            t, n, w, out = timed("k_llr", lambda: dev(method))
            kl.append(t)
            res["launches_k_llr"] = n
            del out
        res["kernel_ms"][method] = {"k_llr_info": ki, "k_llr_info_loss_est_only": ke, "k_llr_llr_only_f32_device": kl}
        res["wall_s"]["run_soft_" + method] = wi
    torch.cuda.empty_cache()

    # the earlier way: every LLR to the host, then NumPy (in slices of realisations: bounded work arrays)
    def host_way():
        w0 = time.perf_counter()
        llr = eng.export_llr(0, SEED, 0, a.reps, fields=("llr",), dtype=np.complex64)["llr"]
        sym = eng.export(0, SEED, 0, a.reps, fields=("sym",))["sym"]
        w1 = time.perf_counter()
        out = np.zeros(llr.shape[1:3] + (2,))
        for r0 in range(0, a.reps, 256):
            bits = ((sym[r0:r0 + 256, None, None, :, None] >> np.arange(m)) & 1).astype(bool)
            loss = bicm_info_loss(llr[r0:r0 + 256], bits).sum(axis=4)
            out[..., 0] += loss.sum(axis=(0, 3))
            out[..., 1] += loss[..., cons].sum(axis=(0, 3))
        return out, w1 - w0, time.perf_counter() - w1

    host_way()
    he, hr = [], []
    for _ in range(a.host_repeats):
        ref, we, wr = host_way()
        he.append(we)
        hr.append(wr)
    res["wall_s"]["export_llr_f32_to_host"] = he
    res["wall_s"]["numpy_reduction"] = hr
    got = soft("exact")["loss_est"]
    res["run_soft_vs_host_f32_rel"] = float(np.abs(got / ref - 1).max())
    res["rate_exact_last_snr_all"] = eng.bicm_rate(0, got, a.reps)[-1, :, 0].tolist()
    res["rate_exact_last_snr_no_edge"] = eng.bicm_rate(0, got, a.reps)[-1, :, 1].tolist()
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
