"""CPU: the host side of dsce_run_soft (DSCE_HAS_SOFT_RUN) — the NumPy reference
dsce.modulation.bicm_info_loss against the literal formula log2(1 + exp(-z)) of
include/dsce.h, its limits, NaN and broadcasting; the header's declaration
against the ctypes binding; and simulate's --rate refusals.  No GPU call.

The literal formula cannot be evaluated in fp64 to 1e-15 relative (at z = 30 the
1 + exp(-z) alone loses 1e-3 of the result), so it is evaluated literally in
60-digit decimal arithmetic and rounded once."""
import ctypes
import decimal
import math
import os
import re
import subprocess

import numpy as np
import pytest

import harness

HDR = os.path.join(harness.ROOT, "include", "dsce.h")


def _literal(z):
    """log2(1 + exp(-z)), the formula as written, in 60 digits."""
    with decimal.localcontext() as ctx:
        ctx.prec = 60
        d = decimal.Decimal(float(z))
        return float((1 + (-d).exp()).ln() / decimal.Decimal(2).ln())


def test_info_loss_against_the_literal_formula():
    from dsce.modulation import bicm_info_loss
    assert bicm_info_loss(0.0, 1) == 1.0 and bicm_info_loss(0.0, 0) == 1.0
    rng = np.random.default_rng(3)
    llr = np.concatenate([rng.uniform(-30, 30, 2000), [-30.0, 30.0, 1e-300, -1e-300, 1e-9, -1e-9],
                          np.arange(-30, 31, dtype=float)])
    for bit in (0, 1):
        z = llr if bit else -llr
        got = bicm_info_loss(llr, bit)
        lit = np.array([_literal(v) for v in z])
        assert got.shape == llr.shape and (lit > 0).all()
        rel = np.abs(got - lit) / lit
        print("info loss, bit %d: worst relative error %.3e" % (bit, rel.max()))
        assert (rel <= 1e-15).all(), rel.max()


def test_info_loss_limits_nan_and_broadcast():
    from dsce.modulation import bicm_info_loss
    ln2 = math.log(2.0)
    # a confident wrong bit: |z| / ln 2, finite; a confident correct one: 0
    for llr, bit in ((1e4, 0), (-1e4, 1)):
        v = float(bicm_info_loss(llr, bit))
        assert np.isfinite(v) and abs(v - 1e4 / ln2) <= 1e-15 * (1e4 / ln2), v
    assert bicm_info_loss(1e4, 1) == 0.0 and bicm_info_loss(-1e4, 0) == 0.0
    assert np.isnan(bicm_info_loss(np.nan, 1)) and np.isnan(bicm_info_loss(np.nan, 0))
    # tends to 0 / grows monotonically
    z = np.linspace(-50, 50, 1001)
    v = bicm_info_loss(z, 1)
    assert (np.diff(v) <= 0).all() and (v >= 0).all() and np.isfinite(v).all()
    # bits broadcast against llr, bool or 0 / 1
    llr = np.random.default_rng(4).standard_normal((3, 2, 5, 4))
    bits = np.array([[0, 1, 1, 0]] * 5)
    out = bicm_info_loss(llr, bits)
    assert out.shape == llr.shape
    for b in range(4):
        assert np.array_equal(out[..., b], bicm_info_loss(llr[..., b], bits[0, b]))
    assert np.array_equal(out, bicm_info_loss(llr, bits.astype(bool)))
    assert np.array_equal(bicm_info_loss(llr, 1), bicm_info_loss(-llr, 0))
    assert bicm_info_loss([1.0, 2.0], [[1], [0]]).shape == (2, 2)


def test_header_declares_run_soft_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    assert re.search(r"^int\s+dsce_run_soft\s*\(", txt, re.M) and "dsce_run_soft" in engine.EXPORTED
    assert re.search(r"^#define DSCE_HAS_SOFT_RUN\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    body = re.search(r"typedef struct \{([^}]*)\} dsce_soft_out;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"double\s*\*\s*(\w+)\s*;", body)
    assert fields == [f for f, _ in engine.SoftOut._fields_] == ["loss_est", "loss_perf0"]
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_SOFT_RUN\n#error "soft run macro"\n#endif\n'
                   'int main(){printf("%zu", sizeof(dsce_soft_out));\n'
                   + "".join('printf(" %%zu", offsetof(dsce_soft_out, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "s"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == [ctypes.sizeof(engine.SoftOut)] + [getattr(engine.SoftOut, f).offset for f in fields]


@pytest.mark.parametrize("extra,word", [(["--checkpoint", "ck.json"], "--checkpoint"),
                                        (["--shard", "snr"], "--shard snr"),
                                        (["--devices", "0,1"], "--devices"),
                                        (["--config", "doubly_flat"], "doubly_flat")])
def test_rate_refusals(extra, word):
    """--rate with a mode it does not cover exits with a message before anything
    touches a GPU (or builds a setup)."""
    from dsce import simulate
    with pytest.raises(SystemExit) as e:
        simulate.main(["--rate", "exact", "--reps", "64"] + extra)
    assert "--rate" in str(e.value) and word in str(e.value), e.value
    with pytest.raises(SystemExit):
        simulate.main(["--rate", "soft"])              # not a method
