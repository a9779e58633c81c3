"""CPU: the host side of the perfect-CSI branch of the soft calls
(DSCE_LLR_PERFECT, DSCE_HAS_LLR_PERFECT) — the header's declarations against the
ctypes binding, the definitions of include/dsce.h closed against the oracle's own
perfect-CSI error counts for all three schemes, and the perfect-CSI LLR arrays
through the shard writer / reader.  No GPU call."""
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from oracle import philox
from test_llr_host import HDR, SEED, demapper_input


def test_header_declares_the_flag_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    assert re.search(r"^#define DSCE_HAS_LLR_PERFECT\s+1\b", txt, re.M)
    assert re.search(r"^#define DSCE_LLR_PERFECT\s+\(1u << 4\)", txt, re.M) and engine.LLR_PERFECT == 1 << 4
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    assert re.search(r"^int\s+dsce_set_llr_scale_perf\s*\(\s*dsce_ctx\s*\*\s*ctx,\s*int32_t\s+scheme_id,\s*"
                     r"const\s+double\s*\*\s*g_perf\s*\)\s*;", txt, re.M)
    assert re.search(r"^int\s+dsce_get_llr_scale_perf\s*\(\s*dsce_ctx\s*\*\s*ctx,\s*int32_t\s+scheme_id,\s*"
                     r"double\s*\*\s*g_perf,\s*int32_t\s*\*\s*set1\s*\)\s*;", txt, re.M)
    for fn in ("dsce_set_llr_scale_perf", "dsce_get_llr_scale_perf"):
        assert fn in engine.EXPORTED
    assert engine.LLR_BRANCHES == {"mmse": 0, "perfect": 1 << 4}
    # the flag is a bit of its own in the shared flags word
    assert len({engine.EXPORT_F32, engine.EXPORT_DEVICE, engine.LLR_MAXLOG, 1 << 3, engine.LLR_PERFECT}) == 5
    src = tmp_path / "p.c"
    src.write_text('#include "dsce.h"\n'
                   '#if !DSCE_HAS_LLR_PERFECT || DSCE_LLR_PERFECT != 16 || DSCE_ABI_VERSION != 10\n'
                   '#error "LLR_PERFECT macros"\n#endif\n'
                   'int (*set_)(dsce_ctx*, int32_t, const double*) = dsce_set_llr_scale_perf;\n'
                   'int (*get_)(dsce_ctx*, int32_t, double*, int32_t*) = dsce_get_llr_scale_perf;\n'
                   'int main(void){return 0;}\n')
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(tmp_path / "p.o")],
                   check=True)
    # the ctypes prototypes, when the library is built (the symbols then exist too)
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        dp, i32p = engine.C.POINTER(engine.C.c_double), engine.C.POINTER(engine.C.c_int32)
        assert lib.dsce_set_llr_scale_perf.argtypes == [engine.C.c_void_p, engine.C.c_int32, dp]
        assert lib.dsce_get_llr_scale_perf.argtypes == [engine.C.c_void_p, engine.C.c_int32, dp, i32p]
    with pytest.raises(ValueError):
        engine.Engine._branch_flag("both")


@pytest.mark.parametrize("name", ["ofdm", "fbmc_aux", "fbmc_cod"])
def test_perfect_definitions_close_on_the_oracle(name):
    """Default scheme, realisations 5..7, SNR (10, 35) dB, n_iter 4: x and pn formed
    by include/dsce.h (demapper_input with h in place of h_est) from
    refsim.simulate's per-unit yperf and h, the host max-log LLR of them, and the
    sign errors against the BITS stream are the oracle's perfect-CSI error counts
    err[0, 1, 0] at every SNR point and stage, exactly.  Every count is >= 18 and
    the smallest margin |LLR pn| is >= 1e-9 (measured on the oracle: 4.0e-6 ofdm,
    8.0e-6 fbmc_aux, 1.6e-6 fbmc_cod)."""
    from dsce.modulation import llr_awgn
    S = harness.setup("default", schemes=(name,), snr_db=(10.0, 35.0), n_iter=4)
    sc = S.schemes[name]
    n, nk, ns, nd, m = 3, 2, S.n_iter + 1, sc["n_data"], sc["bits_per_symbol"]
    tr = {}
    ref = harness.simulate(S, SEED, 5, n, [name], trace=tr)
    LK = sc["G"].shape[1]
    y_perf = np.zeros((n, nk, ns, LK), dtype=complex)
    h = np.zeros_like(y_perf)
    for i in range(n):
        for k in range(nk):
            u = tr["units"][i * nk + k]
            y_perf[i, k] = np.asarray(u["yperf"])
            h[i, k] = np.asarray(u["h"])[None, :]
    x, pe, _ = demapper_input(sc, S.pn_time, y_perf, h)
    assert x.shape == pe.shape == (n, nk, ns, nd) and (pe > 0).all()
    assert np.array_equal(pe, np.broadcast_to(pe[:, :, :1], pe.shape))            # no stage dependence
    if sc["real_detect"]:
        assert not x.imag.any()
    llr = llr_awgn(sc["symbols"], sc["bitmap"], x, pe, "maxlog").reshape(n, nk, ns, nd, m)
    margin = np.abs(llr * pe[..., None]).min()
    print("perfect-CSI margin %s %.3e" % (name, margin))
    assert margin >= 1e-9
    bits = np.stack([philox.bits(SEED, 5 + i, sc["bits_slot"], nd * m).reshape(nd, m) for i in range(n)])
    err = ((llr > 0) != bits[:, None, None].astype(bool)).sum(axis=(0, 3, 4))
    assert ref["err"].shape == (1, 2, 2, nk, ns) and ref["err"][0, 1, 0].min() >= 18
    assert np.array_equal(err, ref["err"][0, 1, 0]), (err, ref["err"][0, 1, 0])


def test_perfect_llr_arrays_round_trip_through_the_shards(tmp_path):
    from dsce import dataset
    rng = np.random.default_rng(3)
    n, nk, S, ND, m = 9, 2, 3, 7, 4
    cplx = lambda: (rng.standard_normal((n, nk, S, ND)) + 1j * rng.standard_normal((n, nk, S, ND))).astype(np.complex64)
    full = dict(sym=rng.integers(0, 16, (n, ND)).astype(np.int32),
                x_est=cplx(), pn_eff=rng.random((n, nk, S, ND)).astype(np.float32),
                llr=rng.standard_normal((n, nk, S, ND, m)).astype(np.float32),
                x_perf=cplx(), pn_perf=rng.random((n, nk, S, ND)).astype(np.float32),
                llr_perf=rng.standard_normal((n, nk, S, ND, m)).astype(np.float32))
    assert dataset.LLR_PERF_ARRAYS == ("x_perf", "pn_perf", "llr_perf")
    assert dataset.LLR_PERF_NAMES == {"x_est": "x_perf", "pn_eff": "pn_perf", "llr": "llr_perf"}
    prefix = str(tmp_path / "set")
    for i, (first, cnt) in enumerate(dataset.shard_ranges(40, n, 4)):
        part = {k: v[first - 40:first - 40 + cnt] for k, v in full.items()}
        dataset.write_shard(dataset.shard_path(prefix, i), part,
                            dict(seed=7, first_rep=first, n_rep=cnt, n_iter=S - 1, llr_method="exact", llr_branch="both"))
    arrays, meta = dataset.read_shard(dataset.shard_path(prefix, 2))
    assert sorted(arrays) == sorted(full) and meta["llr_branch"] == "both" and arrays["llr_perf"].shape == (1, nk, S, ND, m)
    arrays, meta = dataset.load(prefix)
    assert sorted(arrays) == sorted(full)
    for k in full:
        assert arrays[k].dtype == full[k].dtype and np.array_equal(arrays[k], full[k]), k
    assert (meta["first_rep"], meta["n_rep"], meta["llr_branch"]) == (40, n, "both")
    with pytest.raises(ValueError):                 # a perfect-CSI array of another length than the shard
        dataset.write_shard(str(tmp_path / "bad-00000.npz"), {"llr_perf": full["llr_perf"][:3]},
                            dict(seed=7, first_rep=0, n_rep=4))
    # the command line
    ap = dataset.parser()
    assert ap.parse_args(["--reps", "8", "--out", "x", "--llr", "exact"]).llr_branch == "mmse"
    for b in ("mmse", "perfect", "both"):
        assert ap.parse_args(["--reps", "8", "--out", "x", "--llr", "exact", "--llr-branch", b]).llr_branch == b
    with pytest.raises(SystemExit):
        ap.parse_args(["--reps", "8", "--out", "x", "--llr", "exact", "--llr-branch", "none"])
    with pytest.raises(SystemExit):                 # the branch without --llr
        dataset.main(["--reps", "8", "--out", "x", "--llr-branch", "perfect"])
