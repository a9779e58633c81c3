"""CPU: the host side of the bulk per-stage export (dsce_export_stages, ABI 10) —
the header's declaration against the ctypes binding, dsce.dataset.bit_errors
against the oracle's own error counts, and the stage arrays through the shard
writer / reader.  No GPU call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import harness
from oracle import philox

HDR = os.path.join(harness.ROOT, "include", "dsce.h")
SEED = 0x5EED0009


def test_header_declares_export_stages_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    assert re.search(r"^int\s+dsce_export_stages\s*\(", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+%d\b" % engine.ABI_VERSION, txt) and engine.ABI_VERSION == 10
    assert "dsce_export_stages" in engine.EXPORTED
    body = re.search(r"typedef struct \{([^}]*)\} dsce_export_stages_out;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:void|int32_t)\s*\*\s*(\w+)\s*;", body)
    assert fields == [f for f, _ in engine.ExportStagesOut._fields_] == list(engine.STAGE_FIELDS)
    assert fields == ["hp_ls", "h_est", "y_ic", "dec_est", "dec_perf"]
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\nint main(){printf("%zu", '
                   'sizeof(dsce_export_stages_out));\n'
                   + "".join('printf(" %%zu", offsetof(dsce_export_stages_out, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == [ctypes.sizeof(engine.ExportStagesOut)] + [getattr(engine.ExportStagesOut, f).offset for f in fields]


def test_bit_errors_reproduce_the_oracle_counts():
    """dataset.bit_errors of the oracle's own decisions (refsim.simulate's
    per-unit trace, 2 OFDM realisations, 2 SNR points, n_iter 2) against the
    symbols drawn from the BITS stream (bi2de, script:355-357) is the oracle's
    err, exactly, both CSI branches and both edge classes."""
    from dsce import dataset
    S = harness.setup("default", schemes=("ofdm",), snr_db=(10.0, 35.0), n_iter=2)
    sc = S.schemes["ofdm"]
    n, nk, ns, nd, m = 2, 2, S.n_iter + 1, sc["n_data"], sc["bits_per_symbol"]
    tr = {}
    ref = harness.simulate(S, SEED, 5, n, ["ofdm"], trace=tr)
    sym = np.zeros((n, nd), dtype=np.int32)
    for i in range(n):
        b = philox.bits(SEED, 5 + i, sc["bits_slot"], nd * m)
        sym[i] = (b.reshape(nd, m).astype(np.int64) << np.arange(m)).sum(axis=1)
    dec = {k: np.zeros((n, nk, ns, nd), dtype=np.int32) for k in ("dec_e", "dec_p")}
    for i in range(n):
        for k in range(nk):
            u = tr["units"][i * nk + k]
            for key in dec:
                dec[key][i, k] = np.asarray(u[key])
    assert ref["err"].shape == (1, 2, 2, nk, ns) and ref["err"].min() > 0
    for csi, key in enumerate(("dec_e", "dec_p")):
        assert np.array_equal(dataset.bit_errors(sym, dec[key]), ref["err"][0, csi, 0]), key
        assert np.array_equal(dataset.bit_errors(sym, dec[key], considered=sc["considered"]), ref["err"][0, csi, 1]), key
    # a decision nothing formed is refused, and so are mismatched shapes
    bad = dec["dec_e"].copy()
    bad[0, 0, 0, 0] = -1
    with pytest.raises(ValueError):
        dataset.bit_errors(sym, bad)
    with pytest.raises(ValueError):
        dataset.bit_errors(sym[:, :-1], dec["dec_e"])
    # popcount over every bit of the label
    one = dataset.bit_errors(np.array([[0, 255, 5]]), np.array([[[[255, 0, 4]]]]))
    assert one.shape == (1, 1) and one[0, 0] == 17


def test_stage_arrays_round_trip_through_the_shards(tmp_path):
    from dsce import dataset
    rng = np.random.default_rng(1)
    n, nk, S, LK, NP, ND = 11, 2, 3, 12, 3, 9
    cx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    full = dict(y=cx(n, nk, LK), h=cx(n, LK), sym=rng.integers(0, 256, (n, ND)).astype(np.int32),
                hp_ls_stages=cx(n, nk, S, NP), h_est_stages=cx(n, nk, S, LK), y_ic_stages=cx(n, nk, S, LK),
                dec_est=rng.integers(0, 256, (n, nk, S, ND)).astype(np.int32),
                dec_perf=rng.integers(0, 256, (n, nk, S, ND)).astype(np.int32))
    assert set(dataset.STAGE_ARRAYS) <= set(full) and set(dataset.STAGE_NAMES) == {"hp_ls", "h_est", "y_ic", "dec_est",
                                                                                     "dec_perf"}
    prefix = str(tmp_path / "set")
    for i, (first, cnt) in enumerate(dataset.shard_ranges(40, n, 4)):
        part = {k: v[first - 40:first - 40 + cnt] for k, v in full.items()}
        dataset.write_shard(dataset.shard_path(prefix, i), part, dict(seed=7, first_rep=first, n_rep=cnt, n_iter=S - 1))
    arrays, meta = dataset.load(prefix)
    assert sorted(arrays) == sorted(full)
    for k in full:
        assert arrays[k].dtype == full[k].dtype and np.array_equal(arrays[k], full[k]), k
    assert (meta["first_rep"], meta["n_rep"], meta["n_iter"], meta["seed"]) == (40, n, 2, 7)
    with pytest.raises(ValueError):                 # a stage array of another length than the shard
        dataset.write_shard(str(tmp_path / "bad-00000.npz"), {"dec_est": full["dec_est"][:3]},
                            dict(seed=7, first_rep=0, n_rep=4))


def test_cli_stage_flags(capsys):
    from dsce import dataset
    ap = dataset.parser()
    a = ap.parse_args(["--reps", "8", "--out", "x"])
    assert not a.stages and a.n_iter is None
    a = ap.parse_args(["--reps", "8", "--out", "x", "--stages", "--n-iter", "2"])
    assert a.stages and a.n_iter == 2
    for argv in (["--reps", "8", "--out", "x", "--n-iter", "2"], ["--reps", "8", "--out", "x", "--stages", "--no-mmse"]):
        with pytest.raises(SystemExit):
            dataset.main(argv)
    capsys.readouterr()
