"""CPU: the constellation domain of dsce_add_scheme (include/dsce.h at
dsce_scheme_desc.symbols) — the tables of tests/constellations.py are what they
claim to be, the host mirror's own tables keep the spacing rule with a wide
margin, and the slicers' cell-index rule restated in NumPy is the nearest level
exactly on equally spaced axes and not otherwise.  No GPU call; the engine's side
is tests/test_gpu_constellations.py."""
import os
import re

import numpy as np
import pytest

import harness
from constellations import TABLES, grid_table, spacing_deviation, with_constellation

HDR = os.path.join(harness.ROOT, "include", "dsce.h")


def _levels(sym):
    return np.unique(sym.real), np.unique(sym.imag)


def _cell_rule(lv, x):
    """The slicers' rule (nearest_level of kernels_mc.hip): the cell from
    floor((x - lv[0]) / (lv[1] - lv[0])), clamped, then the nearer of its two
    levels, the lower one on a tie."""
    if lv.size == 1:
        return np.zeros(x.shape, dtype=int)
    i = np.clip(np.floor((x - lv[0]) / (lv[1] - lv[0])), 0, lv.size - 2).astype(int)
    return np.where(np.abs(x - lv[i + 1]) < np.abs(x - lv[i]), i + 1, i)


def test_host_mirror_tables_keep_the_spacing_rule():
    """SignalConstellation's QAM 4..256 and PAM 2..16 deviate from equal spacing by
    rounding only: 1e-12 of the span, 1e3 inside the bound dsce_add_scheme applies."""
    from dsce.modulation import SignalConstellation
    for method, orders in (("QAM", (4, 16, 64, 256)), ("PAM", (2, 4, 8, 16))):
        for M in orders:
            lvI, lvQ = _levels(SignalConstellation(M, method).SymbolMapping)
            n = int(np.sqrt(M)) if method == "QAM" else M
            assert lvI.size == n and lvQ.size == (n if method == "QAM" else 1), (method, M)
            assert spacing_deviation(lvI) <= 1e-12 and spacing_deviation(lvQ) <= 1e-12, (method, M)


@pytest.mark.parametrize("tid", list(TABLES))
def test_table_is_what_it_claims(tid):
    T = TABLES[tid]
    sym = grid_table(T.lvI, T.lvQ, T.perm)
    M = T.lvI.size * T.lvQ.size
    assert sym.size == M == 1 << T.m and 1 <= T.m <= 8 and np.all(sym != 0)
    assert abs(np.mean(np.abs(sym) ** 2) - 1.0) <= 1e-14
    lvI, lvQ = _levels(sym)
    assert (lvI.size, lvQ.size) == (T.lvI.size, T.lvQ.size)          # a full rectangular grid
    assert len({(a, b) for a, b in zip(sym.real, sym.imag)}) == M
    assert T.wide == (max(lvI.size, lvQ.size) > 16)
    if T.scheme != "ofdm":
        assert not sym.imag.any()
    dev = max(spacing_deviation(lvI), spacing_deviation(lvQ))
    if tid == "nonuni16":
        assert spacing_deviation(lvI) > 0.1 and spacing_deviation(lvQ) > 0.1
    else:
        assert dev <= 1e-12, dev
    # label bit b of symbol i is (i >> b) & 1: axis-pure for the unpermuted tables, not for the permuted
    bits = (np.arange(M)[:, None] >> np.arange(T.m)) & 1
    alone = lambda b, c: all(len(set(bits[c == v, b])) == 1 for v in np.unique(c))
    pure = all(alone(b, sym.real) or alone(b, sym.imag) for b in range(T.m))
    assert pure == (T.perm is None)


def test_with_constellation_replaces_one_scheme_only():
    S = harness.setup("default", schemes=("ofdm",), snr_db=(15.0, 35.0))
    before = S.schemes["ofdm"]["symbols"].copy()
    S2 = with_constellation(S, "ofdm", 3.0 * grid_table(TABLES["rect32"].lvI, TABLES["rect32"].lvQ))
    sc = S2.schemes["ofdm"]
    assert sc["symbols"].size == 32 and sc["bits_per_symbol"] == 5 and sc["bitmap"].shape == (32, 5)
    assert abs(np.mean(np.abs(sc["symbols"]) ** 2) - 1.0) <= 1e-14
    assert np.array_equal(sc["bitmap"][0b10110], [0, 1, 1, 0, 1])
    assert np.array_equal(S.schemes["ofdm"]["symbols"], before) and S.schemes["ofdm"]["bits_per_symbol"] == 8
    assert sc["G"] is S.schemes["ofdm"]["G"] and S2.pn_time is S.pn_time
    with pytest.raises(AssertionError):
        with_constellation(S, "ofdm", np.array([0.0, 1.0, 2.0, 3.0]))       # a symbol at 0


def test_cell_rule_is_the_nearest_level_only_on_equal_spacing():
    """Why unequal spacing is refused: the slicers' cell-index rule equals the
    argmin over the levels on every equally spaced axis of TABLES (inside and
    outside the grid), and differs from it on a fifth of the draws over nonuni16's
    I axis {-7, -1, 1, 3}."""
    rng = np.random.default_rng(0)
    for tid, T in TABLES.items():
        for lv in (T.lvI, T.lvQ):
            x = rng.uniform(lv[0] - 2.0, lv[-1] + 2.0, 20000)
            ref = np.abs(x[:, None] - lv[None, :]).argmin(axis=1)
            share = float((_cell_rule(lv, x) != ref).mean())
            if tid == "nonuni16":
                # (its Q axis {-3, -1, 1, 7} happens to survive this rule, the wide cell being the
                # clamped last one; the linear slicer of the chain kernels would not)
                assert share > 0.1 or lv is T.lvQ, (tid, share)
            else:
                assert share == 0.0, (tid, share)
    x = rng.uniform(-9.0, 5.0, 100000)
    lv = TABLES["nonuni16"].lvI
    assert 0.19 < (_cell_rule(lv, x) != np.abs(x[:, None] - lv[None, :]).argmin(axis=1)).mean() < 0.23


def test_header_and_readme_state_the_domain():
    txt = open(HDR).read()
    body = re.search(r"const double\* symbols;(.*?)\} dsce_scheme_desc;", txt, re.S).group(1)
    assert "equally" in body and "1e-9" in body and "DSCE_EINVAL" in body
    readme = " ".join(open(os.path.join(harness.ROOT, "README.md")).read().split())
    assert "any number of levels per axis" in readme
