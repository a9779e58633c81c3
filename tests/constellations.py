"""Constellation tables beyond the reference script's, for the tests of the
detector and the demapper (tests/test_constellations_host.py, tests/test_gpu_constellations.py).

dsce_add_scheme takes the constellation as caller data: any power-of-two table
of up to 256 finite symbols that fill a rectangular I x Q grid with equally
spaced levels per axis, under any labelling.  TABLES spans that domain where the
script's square Gray QAM / PAM tables do not reach; with_constellation puts one
of them into the oracle's setup, so oracle and engine read the same table."""
from types import SimpleNamespace

import numpy as np

import harness

SNR = (15.0, 35.0)


def spacing_deviation(lv):
    """max_i |lv[i] - (lv[0] + i (lv[n-1] - lv[0]) / (n-1))| / (lv[n-1] - lv[0]) of
    the sorted levels lv (include/dsce.h at dsce_scheme_desc.symbols: <= 1e-9, for
    n >= 3); 0 for fewer than three levels."""
    lv = np.sort(np.asarray(lv, dtype=float))
    n = lv.size
    if n < 3:
        return 0.0
    span = lv[-1] - lv[0]
    return float(np.abs(lv - (lv[0] + np.arange(n) * span / (n - 1))).max() / span)


def grid_table(lvI, lvQ, perm_seed=None):
    """The points a + 1j b, a in lvI (slow), b in lvQ (fast), scaled to unit mean
    power; perm_seed: permuted by default_rng(perm_seed) (a non-Gray labelling
    whose bits depend on both axes)."""
    s = np.array([a + 1j * b for a in lvI for b in lvQ], dtype=complex)
    s = s / np.sqrt(np.mean(np.abs(s) ** 2))
    if perm_seed is not None:
        s = s[np.random.default_rng(perm_seed).permutation(s.size)]
    return s


def with_constellation(S, name, symbols):
    """A copy of the harness.setup namespace S with scheme `name`'s symbols,
    bits_per_symbol and bitmap replaced (bitmap[i, b] = (i >> b) & 1, the label
    of the C-ABI); the table is scaled to unit mean power.  No symbol may be 0:
    the pilots are symbols[idx] / |symbols[idx]|."""
    sym = np.asarray(symbols, dtype=complex).reshape(-1)
    m = int(np.log2(sym.size))
    assert 1 <= m <= 8 and 1 << m == sym.size, sym.size
    sym = sym / np.sqrt(np.mean(np.abs(sym) ** 2))
    assert np.all(sym != 0), "a pilot would be 0 / 0"
    bm = ((np.arange(sym.size)[:, None] >> np.arange(m)) & 1).astype(np.uint8)
    sc = dict(S.schemes[name], symbols=sym, bits_per_symbol=m, bitmap=bm)
    return SimpleNamespace(**dict(vars(S), schemes=dict(S.schemes, **{name: sc})))


def _odd(n):
    return np.arange(-(n - 1), n, 2.0)                     # n odd-integer levels centred on 0


def _t(lvI, lvQ, scheme="ofdm", perm=None, n_rep=16, n_iter=4):
    lvI, lvQ = np.asarray(lvI, dtype=float), np.asarray(lvQ, dtype=float)
    return SimpleNamespace(scheme=scheme, lvI=lvI, lvQ=lvQ, perm=perm, n_rep=n_rep, n_iter=n_iter,
                           m=int(np.log2(lvI.size * lvQ.size)), wide=max(lvI.size, lvQ.size) > 16)


# id -> grid (levels before scaling), scheme, realisations and IC iterations of the count check.
# wide: more than 16 levels on an axis, which the LDS-table kernels do not take.
TABLES = {
    "bpsk": _t(_odd(2), [0.0]),                            # nQ = 1 without real_detect
    "rect8": _t(_odd(4), _odd(2)),                         # nI != nQ, 3 bits
    "rect32": _t(_odd(8), _odd(4)),                        # 5-bit symbols across words and counters
    "rect128a": _t(_odd(16), _odd(8)),                     # full 16 on one axis only
    "rect128b": _t(_odd(8), _odd(16)),
    "perm64": _t(_odd(8), _odd(8), perm=64),               # non-Gray labellings
    "perm256": _t(_odd(16), _odd(16), perm=256),           # ... and the full-table LLR at M = 256
    "offset16": _t(np.arange(0.0, 4.0), np.arange(1.0, 5.0)),   # lv0 offsets, no symmetry
    "pam32c": _t(_odd(32), [0.0]),                         # more than 16 levels: the fallback slicer
    "rect256a": _t(_odd(32), _odd(8)),
    "rect256b": _t(_odd(8), _odd(32)),
    "fbmc_pam32": _t(_odd(32), [0.0], scheme="fbmc_aux", n_rep=4, n_iter=2),
    "fbmc_pam256": _t(_odd(256), [0.0], scheme="fbmc_aux", n_rep=4, n_iter=2),
    "nonuni16": _t([-7.0, -1.0, 1.0, 3.0], [-3.0, -1.0, 1.0, 7.0]),   # unequal spacing: refused
}


def table_setup(tid):
    """(T, S): TABLES[tid] and the oracle setup (default script parameters, the
    table's scheme alone, SNR (15, 35) dB) holding its constellation."""
    T = TABLES[tid]
    S = harness.setup("default", schemes=(T.scheme,), snr_db=SNR, n_iter=T.n_iter)
    return T, with_constellation(S, T.scheme, grid_table(T.lvI, T.lvQ, T.perm))
