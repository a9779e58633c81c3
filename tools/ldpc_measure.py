"""Measures dsce_run_ldpc (k_ldpc) on one GPU at the C2 export shape of DESIGN.md
section 7k (default config, OFDM, 7 SNR points, n_iter 4, 8192 realisations at
batch 8192), rates 1/2 and 3/4, 30 iterations, alpha 0.75, exact LLRs:

  * kernel time (dsce_kernel_time) of k_ldpc with early stop on and off and of
    k_llr beside it, same process, after a warm-up call, `repeats` calls, the
    best and every value;
  * codewords per second, the mean iterations per SNR point and stage, and the
    time per codeword and iteration they imply;
  * k_viterbi at the same shape from the same run, as the yardstick in the tree;
  * dynamic LDS per block, and VGPRs, SGPRs, static LDS and scratch of the
    instance of k_ldpc that runs (hipcc --cuda-device-only -S, the Makefile's
    flags).

    python tools/ldpc_measure.py --out profiles/ldpc_measure.json

--schedule layered measures dsce_run_ldpc_layered (k_ldpc_layered) over the
first-fit layers of dsce.coding.make_layers in the same way.  --schedule compare
runs, per rate, flooding at the cap --iters, layered at that cap and layered at
half of it (early stop on), one call of each per round so that the three
alternate on the same device, `repeats` rounds after a warm-up round, and
reports for each the kernel ms (best and every value), codewords per second,
mean iterations, ns per codeword and iteration, and BER and FER per SNR point:

    python tools/ldpc_measure.py --schedule compare --out profiles/ldpc_layered_measure.json

--fixed measures dsce_run_ldpc_fixed (k_ldpc_fixed) against dsce_run_ldpc (k_ldpc)
at the same shape: per rate, the fp64 flooding decoder (alpha --alpha) and the
fixed-point one (6 / 6 / 8 bit, scale 2, offset 1; then alpha 3/4 rounded, offset
0) with a real codeword, early stop on, then both without early stop (equal
iteration counts: the per-iteration cost alone), one call of each per round so
that they alternate in one process, `repeats` rounds after a warm-up round.  Per
run: kernel ms (best and every value), codewords per second, mean iterations,
ns per codeword and iteration, BER and FER per SNR point.  Then, under
"fer_study", FER, BER and mean iterations at the last stage per SNR point of the
fp64 decoder and of fixed-point ones at four channel clips C / scale, a 4-bit
one, and two rows with the all-zero word in place of the real codeword:

    python tools/ldpc_measure.py --fixed --out profiles/ldpc_fixed_measure.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch          # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "channel-estimation_amd")
sys.path[:0] = [PKG]

SEED = 0x5EED0002
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def kernel_resources(vpt=None, kernel="k_ldpc"):
    """.amdhsa_* of `kernel`: k_ldpc (its instance <vpt>), k_ldpc_layered or k_ldpc_fixed"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    unit = {"k_ldpc": "kernels_ldpc.hip", "k_ldpc_layered": "kernels_ldpc_layered.hip", "k_ldpc_fixed": "kernels_ldpc_fixed.hip"}[kernel]
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                                          "--cuda-device-only", "-S", os.path.join(PKG, "csrc", unit),
                                          "-o", out], check=True, capture_output=True)
        txt = open(out).read()
    name = {"k_ldpc": r"6k_ldpcILi%sE" % vpt, "k_ldpc_layered": "14k_ldpc_layeredE", "k_ldpc_fixed": "12k_ldpc_fixedE"}[kernel]
    m = re.search(r"\.amdhsa_kernel (\S*%s\S*)\n(.*?)\.end_amdhsa_kernel" % name, txt, re.S)
    f = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
    return {"kernel": m.group(1), "vgprs": int(f["next_free_vgpr"]), "sgprs": int(f["next_free_sgpr"]),
            "lds_static_bytes": int(f["group_segment_fixed_size"]), "scratch_bytes": int(f["private_segment_fixed_size"])}


def fixed_thread_cap():
    """DSCE_LDPC_FIXED_MAX_THREADS as kernels_ldpc_fixed.hip defines it, or as DSCE_LDPC_FIXED_MAX_THREADS in the
    environment says for a library built with the macro overridden"""
    if os.environ.get("DSCE_LDPC_FIXED_MAX_THREADS"):
        return int(os.environ["DSCE_LDPC_FIXED_MAX_THREADS"])
    txt = open(os.path.join(PKG, "csrc", "kernels_ldpc_fixed.hip")).read()
    return int(re.search(r"^#define DSCE_LDPC_FIXED_MAX_THREADS\s+(\d+)", txt, re.M).group(1))


def layer_shape(code, layers):
    """the lanes k_ldpc_layered gives each layer: a check takes the power of two >= its degree, a layer a multiple of 64"""
    lp, lc = layers
    deg = np.diff(code.row_ptr)
    lanes = [-(-sum(max(2, 1 << int(d - 1).bit_length()) for d in deg[lc[lp[l]:lp[l + 1]]]) // 64) * 64
             for l in range(lp.size - 1)]
    return {"n_layers": int(lp.size - 1), "checks_per_layer": np.diff(lp).tolist(), "lanes_per_layer": lanes,
            "threads_per_block_layered": min(1024, max(lanes))}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--schedule", choices=("flooding", "layered", "compare"), default="flooding")
    ap.add_argument("--fixed", action="store_true", help="k_ldpc_fixed against k_ldpc, alternating (see above)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    if a.fixed:
        a.schedule = "fixed"

    from dsce.coding import ldpc_encode, ldpc_fixed_lds_bytes, make_code, make_fixed, make_layers, make_ldpc
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=a.batch)
    sc = S.schemes["ofdm"]
    B = int(sc.n_data) * int(sc.bits_per_symbol)
    nk, ns = len(S.snr_db), int(S.n_iter) + 1
    ncw = a.reps * nk * ns
    res = {"config": "default", "scheme": "ofdm", "n_snr": nk, "snr_db": [float(x) for x in S.snr_db],
           "n_iter": int(S.n_iter), "slots": B, "reps": a.reps, "batch": a.batch,
           "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "method": "exact", "codewords": ncw,
           "max_iter": a.iters, "alpha": a.alpha, "lds_max": eng.get_option("lds_max"), "schedule": a.schedule,
           "rates": {}}
    layered = a.schedule == "layered"
    kname = "k_ldpc_layered" if layered else "k_ldpc"

    def timed(fn, names):
        eng.enable_timing(True)
        before = {k: eng.kernel_time(k) for k in names}
        w0 = time.perf_counter()
        out = fn()
        w = time.perf_counter() - w0
        after = {k: eng.kernel_time(k) for k in before}
        eng.enable_timing(False)
        return {k: after[k][1] - before[k][1] for k in before}, w, out

    def entry(code, out, kd):
        best = min(kd)
        iters = float(out["iter_sum"].sum())
        return {"max_iter": int(code.max_iter), "kernel_ms": kd, "kernel_ms_best": best,
                "codewords_per_s": ncw / (best * 1e-3), "mean_iter": (out["iter_sum"] / float(a.reps)).tolist(),
                "mean_iter_all": iters / ncw, "ns_per_codeword_iteration": best * 1e6 / iters,
                "ber": (out["bit_err"] / (a.reps * float(code.n_info))).tolist(),
                "fer": (out["frame_err"] / float(a.reps)).tolist()}

    for rate in ("1/2", "3/4") if a.schedule == "fixed" else ():
        code = make_ldpc(B, rate, max_iter=a.iters, alpha=a.alpha)
        full = code._replace(early_stop=False)
        word = ldpc_encode(np.random.RandomState(11).randint(0, 2, code.n_info), code)
        offset = make_fixed()
        norm = make_fixed(6, 6, 8, scale=2.0, alpha_num=3, alpha_shift=2, beta=0)
        runs = [("fp64", code, None, "k_ldpc"), ("fixed_offset1", code, offset, "k_ldpc_fixed"),
                ("fixed_alpha3_4", code, norm, "k_ldpc_fixed"), ("fp64_all_iterations", full, None, "k_ldpc"),
                ("fixed_all_iterations", full, offset, "k_ldpc_fixed")]
        kd, outs = {k: [] for k, _, _, _ in runs}, {}
        for rnd in range(a.repeats + 1):                     # round 0 warms up (buffers, clocks, code objects)
            for key, c, fx, name in runs:
                ms, w, outs[key] = timed(lambda: eng.run_ldpc(0, SEED, 0, a.reps, c, fixed=fx,
                                                              codeword=word if fx is not None else None), (name,))
                if rnd:
                    kd[key].append(ms[name])
        r = {key: entry(c, outs[key], kd[key]) for key, c, fx, name in runs}
        for key, c, fx, name in runs:
            r[key]["fixed"] = dict(fx._asdict()) if fx is not None else None
        r["fixed_over_fp64"] = {"early_stop": r["fixed_offset1"]["kernel_ms_best"] / r["fp64"]["kernel_ms_best"],
                                "all_iterations": r["fixed_all_iterations"]["kernel_ms_best"] /
                                r["fp64_all_iterations"]["kernel_ms_best"]}
        r.update({"info_bits": code.n_info, "n_checks": code.n_checks, "edges": int(code.col.size),
                  "lds_dynamic_bytes_per_block": {"k_ldpc": 8 * code.n_vars + 24 * code.n_checks + 8,
                                                  "k_ldpc_fixed": ldpc_fixed_lds_bytes(code.n_vars, code.n_checks)},
                  "threads_per_block_fixed": min(fixed_thread_cap(), (max(code.n_vars, code.n_checks) + 63) // 64 * 64)})
        # what the word length costs on this channel: FER / BER / iterations at the last stage, per SNR point, of the
        # fp64 decoder and of fixed-point ones at three channel clips C / scale, one 4-bit decoder, and one row with
        # the all-zero word in place of the real codeword (optimistic at ties: include/dsce.h)
        study = [("fp64 alpha %g" % a.alpha, None, None),
                 ("6/6/8 offset 1, clip 124", make_fixed(6, 6, 8, scale=0.25), word),
                 ("6/6/8 offset 1, clip 31", make_fixed(6, 6, 8, scale=1.0), word),
                 ("6/6/8 offset 1, clip 15.5", offset, word),
                 ("6/6/8 offset 1, clip 7.75", make_fixed(6, 6, 8, scale=4.0), word),
                 ("6/6/8 alpha 3/4, clip 15.5", norm, word),
                 ("4/4/6 offset 1, clip 7", make_fixed(4, 4, 6, scale=1.0), word),
                 ("4/4/6 offset 1, clip 7, all-zero word", make_fixed(4, 4, 6, scale=1.0), None),
                 ("6/6/8 offset 1, clip 15.5, all-zero word", offset, None)]
        r["fer_study"] = {}
        for label, fx, w in study:
            o = outs["fp64"] if fx is None else outs["fixed_offset1"] if (fx is offset and w is word) else \
                outs["fixed_alpha3_4"] if fx is norm else eng.run_ldpc(0, SEED, 0, a.reps, code, fixed=fx, codeword=w)
            r["fer_study"][label] = {"fixed": dict(fx._asdict()) if fx is not None else None,
                                     "real_codeword": w is not None if fx is not None else None,
                                     "fer_last_stage": (o["frame_err"][:, -1] / float(a.reps)).tolist(),
                                     "ber_last_stage": (o["bit_err"][:, -1] / (a.reps * float(code.n_info))).tolist(),
                                     "mean_iter_last_stage": (o["iter_sum"][:, -1] / float(a.reps)).tolist()}
        try:
            r["k_ldpc_fixed_resources"] = kernel_resources(kernel="k_ldpc_fixed")
        except Exception as e:
            r["k_ldpc_fixed_resources"] = {"error": str(e)[:200]}
        res["rates"][rate] = r
    for rate in ("1/2", "3/4") if a.schedule == "compare" else ():
        code = make_ldpc(B, rate, max_iter=a.iters, alpha=a.alpha)
        layers = make_layers(code)
        half = code._replace(max_iter=max(1, a.iters // 2))
        runs = [("flooding", code, None, "k_ldpc"), ("layered", code, layers, "k_ldpc_layered"),
                ("layered_half_cap", half, layers, "k_ldpc_layered")]
        kd, outs = {k: [] for k, _, _, _ in runs}, {}
        for rnd in range(a.repeats + 1):                     # round 0 warms up (buffers, clocks, code objects)
            for key, c, ly, name in runs:
                ms, w, outs[key] = timed(lambda: eng.run_ldpc(0, SEED, 0, a.reps, c, layers=ly), (name,))
                if rnd:
                    kd[key].append(ms[name])
        r = {key: entry(c, outs[key], kd[key]) for key, c, ly, name in runs}
        r.update({"info_bits": code.n_info, "n_checks": code.n_checks, "edges": int(code.col.size),
                  "lds_dynamic_bytes_per_block": 8 * code.n_vars + 24 * code.n_checks + 8})
        r.update(layer_shape(code, layers))
        try:
            r["k_ldpc_layered_resources"] = kernel_resources(kernel="k_ldpc_layered")
        except Exception as e:
            r["k_ldpc_layered_resources"] = {"error": str(e)[:200]}
        res["rates"][rate] = r
    for rate in ("1/2", "3/4") if a.schedule in ("flooding", "layered") else ():
        r = {}
        for early in (1, 0):
            code = make_ldpc(B, rate, max_iter=a.iters, alpha=a.alpha, early_stop=bool(early))
            layers = make_layers(code) if layered else None
            run = lambda: eng.run_ldpc(0, SEED, 0, a.reps, code, layers=layers)
            run()                                            # warm-up (buffers, clocks, code objects)
            kd, kl, wall = [], [], []
            for _ in range(a.repeats):
                ms, w, out = timed(run, (kname, "k_llr"))
                kd.append(ms[kname])
                kl.append(ms["k_llr"])
                wall.append(w)
            best = min(kd)
            iters = float(out["iter_sum"].sum())
            r["early_stop" if early else "all_iterations"] = {
                "k_ldpc_ms": kd, "k_ldpc_ms_best": best, "k_llr_ms": kl, "wall_s": wall,
                "codewords_per_s": ncw / (best * 1e-3),
                "mean_iter": (out["iter_sum"] / float(a.reps)).tolist(),
                "mean_iter_all": iters / ncw,
                # each codeword also spends one check phase more than its iterations where it stops early
                "us_per_codeword_iteration": best * 1e3 / iters,
                "ber": (out["bit_err"] / (a.reps * float(code.n_info))).tolist(),
                "fer": (out["frame_err"] / float(a.reps)).tolist()}
        nt = min(1024, (max(code.n_vars, code.n_checks) + 63) // 64 * 64)
        vpt = -(-code.n_vars // nt)
        vpt = next(v for v in (1, 2, 4, 8, 16, 0) if v == 0 or vpt <= v)
        r.update({"info_bits": code.n_info, "n_checks": code.n_checks, "edges": int(code.col.size),
                  "four_cycles": code.four_cycles, "threads_per_block": nt, "variables_per_thread": vpt,
                  "lds_dynamic_bytes_per_block": 8 * code.n_vars + 24 * code.n_checks + 8})
        try:
            r["k_ldpc_resources"] = kernel_resources(vpt, kname)
            if layered:
                r.update(layer_shape(code, layers))
        except Exception as e:                               # no compiler here: the run is still measured
            r["k_ldpc_resources"] = {"error": str(e)[:200]}
        conv = make_code(B, rate, interleaver=7)
        runv = lambda: eng.run_coded(0, SEED, 0, a.reps, conv)
        runv()
        kv = [timed(runv, ("k_viterbi",))[0]["k_viterbi"] for _ in range(a.repeats)]
        r["k_viterbi_ms"] = kv
        r["k_ldpc_over_k_viterbi"] = {k: r[k]["k_ldpc_ms_best"] / min(kv) for k in ("early_stop", "all_iterations")}
        res["rates"][rate] = r
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
