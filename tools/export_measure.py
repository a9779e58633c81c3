"""Measures the bulk export (dsce_export / k_export) on one GPU at the C2 shapes
a user would export: default config, OFDM, 7 SNR points,
65536 realisations in batches of 8192, device destination (torch tensors).

  * k_export's kernel time (dsce_kernel_time) against a device-to-device copy
    of the same number of output bytes, timed in the same process and
    alternating with it; the copy's repeat-to-repeat spread is the margin;
  * the same for single-field exports, which separate the pure transpose (y),
    the LS estimates (hp_ls) and the Wd hP product (h_est);
  * the end-to-end export rate (Jakes, TX and receiver front included) next to
    a loop of dsce_trace_unit_ex calls, the only earlier way to the same data;
  * the host-destination rate (PCIe-inclusive: staging buffer + copy back).

    python tools/export_measure.py --out profiles/r07_export.json
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
FIELDS = ("y", "hp_ls", "h_est", "h", "xp", "sym")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--host-reps", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from dsce.configs import build_setup
    from dsce.engine import EXPORT_DEVICE, EXPORT_F32, build_engine, gpu_tx
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=a.batch)
    res = {"config": "default", "scheme": "ofdm", "n_snr": len(S.snr_db), "reps": a.reps, "batch": a.batch,
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "dtypes": {}}

    def kernel_ms(fn):
        """fn() with timing on: (k_export ms, wall s) of that call alone."""
        eng.enable_timing(True)
        n0, t0 = eng.kernel_time("k_export")
        w0 = time.perf_counter()
        fn()
        w = time.perf_counter() - w0
        n1, t1 = eng.kernel_time("k_export")
        eng.enable_timing(False)
        return t1 - t0, w, n1 - n0

    def copy_ms(nbytes, src, dst):
        a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a_.record()
        dst[:nbytes].copy_(src[:nbytes])
        b_.record()
        torch.cuda.synchronize()
        return a_.elapsed_time(b_)

    for name in ("complex64", "complex128"):
        dt = getattr(torch, name)
        flags = EXPORT_DEVICE | (EXPORT_F32 if name == "complex64" else 0)
        shapes = eng.export_shapes(0, a.reps)
        out = {f: torch.empty(shapes[f], dtype=torch.int32 if f == "sym" else dt, device="cuda:0") for f in FIELDS}
        nbytes = {f: t.numel() * t.element_size() for f, t in out.items()}
        total = sum(nbytes.values())
        src = torch.empty(total, dtype=torch.uint8, device="cuda:0").random_(0, 256)
        dst = torch.empty(total, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def export(fields):
            eng._export(0, SEED, 0, a.reps, flags, {f: out[f].data_ptr() for f in fields})

        export(FIELDS)                                    # warm-up (buffers, clocks)
        copy_ms(total, src, dst)
        r = {"bytes": nbytes, "bytes_total": total, "all": [], "copy_all": [], "wall_s": [], "parts": {}}
        for _ in range(a.repeats):                        # alternating
            k, w, n = kernel_ms(lambda: export(FIELDS))
            r["all"].append(k)
            r["wall_s"].append(w)
            r["launches"] = n
            r["copy_all"].append(copy_ms(total, src, dst))
        for f in ("y", "hp_ls", "h_est"):
            ks, cs = [], []
            for _ in range(a.repeats):
                ks.append(kernel_ms(lambda: export((f,)))[0])
                cs.append(copy_ms(nbytes[f], src, dst))
            r["parts"][f] = {"k_export_ms": ks, "copy_ms": cs, "ratio_of_medians": float(np.median(ks) / np.median(cs))}
        kmed, cmed = float(np.median(r["all"])), float(np.median(r["copy_all"]))
        r["k_export_ms_median"] = kmed
        r["copy_ms_median"] = cmed
        r["copy_spread_rel"] = float((max(r["copy_all"]) - min(r["copy_all"])) / cmed)
        r["ratio_k_export_over_copy"] = kmed / cmed
        r["k_export_write_GBps"] = total / kmed / 1e6
        r["copy_GBps_one_way"] = total / cmed / 1e6
        r["export_realisations_per_s"] = a.reps / float(np.median(r["wall_s"]))
        # host destination (PCIe-inclusive)
        eng.export(0, SEED, 0, a.host_reps, dtype=np.dtype(name))
        hw = []
        for _ in range(3):
            t0 = time.perf_counter()
            eng.export(0, SEED, 0, a.host_reps, dtype=np.dtype(name))
            hw.append(time.perf_counter() - t0)
        r["host_reps"] = a.host_reps
        r["host_wall_s"] = hw
        r["host_realisations_per_s_pcie_inclusive"] = a.host_reps / float(np.median(hw))
        res["dtypes"][name] = r
        del out, src, dst
        torch.cuda.empty_cache()

    # the earlier way: one dsce_trace_unit_ex per (realisation, SNR) unit
    eng.trace_unit(0, SEED, 0, 0)
    t0 = time.perf_counter()
    for i in range(64):
        eng.trace_unit(0, SEED, i // len(S.snr_db), i % len(S.snr_db))
    tw = time.perf_counter() - t0
    res["trace_unit"] = {"units": 64, "wall_s": tw, "units_per_s": 64 / tw,
                         "realisations_per_s": 64 / tw / len(S.snr_db)}
    for name, r in res["dtypes"].items():
        r["speedup_over_trace_unit_loop"] = r["export_realisations_per_s"] / res["trace_unit"]["realisations_per_s"]
    eng.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
