"""Measures dsce_run_coded (k_viterbi) on one GPU at the C2 export shape of
DESIGN.md section 7g (default config, OFDM, 7 SNR points, n_iter 4, 8192
realisations at batch 8192), rates 1/2 and 3/4, exact LLRs:

  * kernel time (dsce_kernel_time) of k_viterbi and of k_llr beside it (the fp64
    LLRs the decoder reads), same process, after a warm-up call, `repeats` calls;
  * codewords per second of k_viterbi, cycles per trellis step and wave, and the
    wall time of run_coded;
  * VGPRs, SGPRs, static LDS and scratch of k_viterbi from the device assembly
    (hipcc --cuda-device-only -S, the Makefile's flags), and its dynamic LDS.

    python tools/coded_measure.py --out profiles/coded_measure.json
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import torch          # before the engine's library: one HIP runtime for both

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "channel-estimation_amd")
sys.path[:0] = [PKG]

SEED = 0x5EED0002
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-ffp-contract=off", "-mllvm", "-amdgpu-mfma-vgpr-form=1"]


def kernel_resources(name="k_viterbi"):
    """.amdhsa_* of the kernel whose mangled name contains `name` followed by a non-identifier character"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([hipcc] + FLAGS + ["-I", os.path.join(ROOT, "include"), "-I", os.path.join(PKG, "csrc"),
                                          "--cuda-device-only", "-S", os.path.join(PKG, "csrc", "kernels_viterbi.hip"),
                                          "-o", out], check=True, capture_output=True)
        txt = open(out).read()
    m = re.search(r"\.amdhsa_kernel (\S*%s[A-Z]\S*)\n(.*?)\.end_amdhsa_kernel" % name, txt, re.S)
    f = dict(re.findall(r"\.amdhsa_(\w+) (\S+)", m.group(2)))
    return {"kernel": m.group(1), "vgprs": int(f["next_free_vgpr"]), "sgprs": int(f["next_free_sgpr"]),
            "lds_static_bytes": int(f["group_segment_fixed_size"]), "scratch_bytes": int(f["private_segment_fixed_size"])}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--clock-mhz", type=float, default=2400.0,
                    help="engine clock for the cycles-per-step figure (MI355X peak: 2400)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)

    from dsce.coding import make_code
    from dsce.configs import build_setup
    from dsce.engine import build_engine, gpu_tx
    S = build_setup("default", schemes=("ofdm",), tx=gpu_tx(0))
    eng = build_engine(S, batch=a.batch)
    sc = S.schemes["ofdm"]
    B = int(sc.n_data) * int(sc.bits_per_symbol)
    nk, ns = len(S.snr_db), int(S.n_iter) + 1
    prop = torch.cuda.get_device_properties(0)
    res = {"config": "default", "scheme": "ofdm", "n_snr": nk, "n_iter": int(S.n_iter), "slots": B, "reps": a.reps,
           "batch": a.batch, "device": torch.cuda.get_device_name(0), "repeats": a.repeats, "method": "exact",
           "codewords": a.reps * nk * ns, "rates": {}}
    try:
        res["k_viterbi_resources"] = kernel_resources()
    except Exception as e:                                   # no compiler here: the run is still measured
        res["k_viterbi_resources"] = {"error": str(e)[:200]}

    def timed(fn):
        eng.enable_timing(True)
        before = {k: eng.kernel_time(k) for k in ("k_viterbi", "k_llr")}
        w0 = time.perf_counter()
        out = fn()
        w = time.perf_counter() - w0
        after = {k: eng.kernel_time(k) for k in before}
        eng.enable_timing(False)
        return {k: after[k][1] - before[k][1] for k in before}, {k: after[k][0] - before[k][0] for k in before}, w, out

    for rate in ("1/2", "3/4"):
        code = make_code(B, rate, interleaver=7)
        run = lambda: eng.run_coded(0, SEED, 0, a.reps, code)
        run()                                                # warm-up (buffers, clocks, code objects)
        kv, kl, wall = [], [], []
        for _ in range(a.repeats):
            ms, n, w, out = timed(run)
            kv.append(ms["k_viterbi"])
            kl.append(ms["k_llr"])
            wall.append(w)
        best = min(kv)
        wpb = max(1, min(4, 8192 // code.n_steps))
        waves = res["codewords"]
        # SIMD cycles spent per trellis step and wave at the peak clock: time x clock x SIMDs / (waves x steps)
        simds = prop.multi_processor_count * 4
        clk_hz = a.clock_mhz * 1e6
        r = {"steps": code.n_steps, "info_bits": code.n_info, "k_viterbi_ms": kv, "k_llr_ms": kl, "wall_s": wall,
             "launches": n, "codewords_per_s": waves / (best * 1e-3), "waves_per_block": wpb,
             "lds_dynamic_bytes_per_block": wpb * code.n_steps * 8,
             "ber": (out["bit_err"] / (a.reps * float(code.n_info))).tolist(), "fer": (out["frame_err"] / float(a.reps)).tolist()}
        if clk_hz:
            r["simd_cycles_per_step_and_wave"] = best * 1e-3 * clk_hz * simds / (waves * code.n_steps)
            r["clock_mhz"] = clk_hz / 1e6
        res["rates"][rate] = r
    eng.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
