"""CPU: the host side of the bulk export (dsce_export, ABI 9) — the header's
declaration against the ctypes binding, and the shard writer / reader and the
argument parser of dsce.dataset.  No GPU call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import harness

HDR = os.path.join(harness.ROOT, "include", "dsce.h")


def test_header_declares_export_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    assert re.search(r"^int\s+dsce_export\s*\(", txt, re.M)
    assert "dsce_export" in engine.EXPORTED and engine.ABI_VERSION >= 9
    assert re.search(r"#define DSCE_ABI_VERSION\s+%d\b" % engine.ABI_VERSION, txt)
    for name, val in (("F32", engine.EXPORT_F32), ("DEVICE", engine.EXPORT_DEVICE)):
        m = re.search(r"#define DSCE_EXPORT_%s\s+\(1u << (\d+)\)" % name, txt)
        assert m and 1 << int(m.group(1)) == val, name
    # the struct: the header's field order, and the C compiler's size / offsets
    body = re.search(r"typedef struct \{([^}]*)\} dsce_export_out;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(?:void|int32_t)\s*\*\s*(\w+)\s*;", body)
    assert fields == [f for f, _ in engine.ExportOut._fields_] == list(engine.EXPORT_FIELDS)
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\nint main(){printf("%zu", '
                   'sizeof(dsce_export_out));\n'
                   + "".join('printf(" %%zu", offsetof(dsce_export_out, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == [ctypes.sizeof(engine.ExportOut)] + [getattr(engine.ExportOut, f).offset for f in fields]


def _synthetic(n, nsnr=2, LK=12, NP=3, ND=9, dtype=np.complex64, seed=0):
    rng = np.random.default_rng(seed)
    cx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(dtype)
    return dict(y=cx(n, nsnr, LK), hp_ls=cx(n, nsnr, NP), h_est=cx(n, nsnr, LK), h=cx(n, LK), xp=cx(n, NP),
                sym=rng.integers(0, 256, (n, ND)).astype(np.int32))


def test_shards_round_trip_with_ragged_tail(tmp_path):
    from dsce import dataset
    full = _synthetic(23)
    base = dict(config="default", scheme="ofdm", snr_db=np.array([10.0, 35.0]), pn_time=np.array([1e-1, 3e-4]),
                seed=(1 << 63) + 5, dtype="complex64", pilot_pos=np.arange(3, dtype=np.int32),
                data_pos=np.arange(3, 12, dtype=np.int32), symbols=np.exp(1j * np.arange(4)), kappa=2.0,
                data_div=1.5, L=4, K=3, abi=9)
    prefix = str(tmp_path / "sub" / "set")
    ranges = dataset.shard_ranges(100, 23, 10)
    assert ranges == [(100, 10), (110, 10), (120, 3)]
    for i, (first, n) in enumerate(ranges):
        part = {k: v[first - 100:first - 100 + n] for k, v in full.items()}
        p = dataset.write_shard(dataset.shard_path(prefix, i), part, dict(base, first_rep=first, n_rep=n))
        assert p.endswith("set-%05d.npz" % i) and os.path.exists(p)
    assert sorted(os.listdir(tmp_path / "sub")) == ["set-00000.npz", "set-00001.npz", "set-00002.npz"]
    a, m = dataset.read_shard(dataset.shard_path(prefix, 2))
    assert m["first_rep"] == 120 and m["n_rep"] == 3 and a["y"].shape == (3, 2, 12)
    arrays, meta = dataset.load(prefix)
    assert sorted(arrays) == sorted(full)
    for k in full:
        assert arrays[k].dtype == full[k].dtype and np.array_equal(arrays[k], full[k]), k
    assert meta["first_rep"] == 100 and meta["n_rep"] == 23
    assert meta["config"] == "default" and meta["scheme"] == "ofdm" and meta["dtype"] == "complex64"
    assert meta["seed"] == (1 << 63) + 5 and meta["abi"] == 9 and (meta["L"], meta["K"]) == (4, 3)
    assert meta["kappa"] == 2.0 and meta["data_div"] == 1.5
    for k in ("snr_db", "pn_time", "pilot_pos", "data_pos", "symbols"):
        assert np.array_equal(meta[k], base[k]), k


def test_shard_writer_and_loader_reject_inconsistent_sets(tmp_path):
    from dsce import dataset
    part = _synthetic(4)
    with pytest.raises(ValueError):
        dataset.write_shard(str(tmp_path / "a-00000.npz"), part, dict(first_rep=0, n_rep=5, seed=1))
    with pytest.raises(ValueError):
        dataset.write_shard(str(tmp_path / "a-00000.npz"), {"bogus": part["y"]}, dict(first_rep=0, n_rep=4, seed=1))
    prefix = str(tmp_path / "gap")
    dataset.write_shard(dataset.shard_path(prefix, 0), part, dict(first_rep=0, n_rep=4, seed=1))
    dataset.write_shard(dataset.shard_path(prefix, 1), part, dict(first_rep=5, n_rep=4, seed=1))
    with pytest.raises(ValueError):
        dataset.load(prefix)
    with pytest.raises(FileNotFoundError):
        dataset.load(str(tmp_path / "none"))
    assert dataset.shard_ranges(7, 0, 4) == []


def test_cli_accepts_only_the_two_dtypes(capsys):
    from dsce import dataset
    ap = dataset.parser()
    for dt in dataset.DTYPES:
        assert ap.parse_args(["--reps", "8", "--out", "x", "--dtype", dt]).dtype == dt
    assert dataset.DTYPES == ("complex64", "complex128")
    for bad in ("float32", "complex32", "c64"):
        with pytest.raises(SystemExit):
            ap.parse_args(["--reps", "8", "--out", "x", "--dtype", bad])
    capsys.readouterr()
    a = ap.parse_args(["--reps", "96", "--shard-reps", "64", "--snr-db", "10", "35", "--out", "x", "--no-mmse"])
    assert a.snr_db == [10.0, 35.0] and a.no_mmse and a.shard_reps == 64
