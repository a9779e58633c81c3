"""Frame geometries beyond the reference script's, for the tests of everything
behind dsce_add_scheme that branches on the frame (tests/test_geometries_host.py,
tests/test_gpu_geometries.py).

dsce_add_scheme takes the frame as caller data: any n_subcarriers x n_symbols,
any N, 1 <= n_pilots <= 64 pilots at any positions (include/dsce.h at
dsce_scheme_desc).  oracle/setup.py::script_setup builds three frames with
hard-coded pilot matrices (NP 16 or 32, LK a multiple of 24); GEOMETRIES spans
the domain where those do not reach: NP off a multiple of 4 (1, 5), NP / 4 = 3,
NP 8 and 32 on 24-row blocks, NP 8 and 16 on 32-row blocks (FBMC), NP up to 64,
LK with a partial row block, blocks that straddle OFDM symbols, ND off a
multiple of 32, FBMC off L = 24 / 48.

ofdm_scheme / fbmc_scheme restate script_setup's two scheme builders for any
pilot matrix, from the oracle's own classes only (tests/test_geometries_host.py
shows they return script_setup("default")'s dicts array for array when fed the
script's matrices); geometry_setup wraps one scheme into the namespace
harness.setup returns, so harness.engine, harness.simulate and
harness.oracle_mmse work on it unchanged."""
import functools
from types import SimpleNamespace

import numpy as np

import harness  # noqa: F401  (puts the repository root on sys.path)
from oracle import setup as osu

F = 15e3
SNR = (15.0, 35.0)
P2D, P2D_AUX, P2D_COD = 2.0, 4.685, 4.0
RINV_LDS_LIMIT = 64 * 1024            # k_rinv keeps its matrices in LDS up to here (kernels_setup.hip)


def rinv_lds_bytes(n_pilots):
    """Dynamic LDS of k_rinv's in-LDS form: the NP x 2NP augmented matrix and the
    NP x NP residual of the refinement, 16 B each."""
    return n_pilots * 3 * n_pilots * 16


def pilot_matrix(L, K, pilots):
    pm = np.zeros((L, K))
    for l, k in pilots:
        assert 0 <= l < L and 0 <= k < K and pm[l, k] == 0, (l, k)
        pm[l, k] = 1
    return pm


def ofdm_scheme(of, pm, cons, qam, p2d=P2D):
    """script_setup's "ofdm" dict (oracle/setup.py, `if "ofdm" in schemes`) for the
    modulator `of`, pilot matrix pm (L x K, 1 at a pilot) and edge mask cons."""
    pmv = osu.col(pm)
    LK = pmv.size
    NP = int(np.sum(pm == 1))
    ND = int(np.sum(pm == 0))
    Pm = np.zeros((LK, LK))
    Pm[np.ix_(pmv == 1, np.arange(NP))] = np.sqrt(p2d) * np.eye(NP)
    Pm[np.ix_(pmv == 0, np.arange(NP, LK))] = np.eye(ND)
    Pm = Pm / np.sqrt(np.mean(np.diag(Pm @ Pm.T)))
    dpr = LK / (NP * p2d + ND)
    sel = (osu.col(cons) * (pmv == 0)) == 1
    cm = np.array([np.sum(np.abs(Pm[sel, NP + i])) > dpr * 0.9 for i in range(ND)])
    return dict(G=of.tx_matrix(), Q=of.rx_matrix().conj().T, P=Pm.astype(complex),
                pilot_pos=np.flatnonzero(pmv == 1), data_pos=np.flatnonzero(pmv == 0), despread=False,
                real_detect=False, data_div=float(np.sqrt(dpr)), kappa=float(p2d * dpr), symbols=qam[0],
                bitmap=qam[1].astype(np.uint8), bits_per_symbol=qam[1].shape[1], n_data=ND,
                considered=cm, bits_slot=2, pilot_slot=1)


def fbmc_scheme(fb, pm, cons, pam, method):
    """script_setup's "fbmc_aux" ("Auxiliary") or "fbmc_cod" ("Coding") dict for
    the modulator fb, pilot matrix pm and edge mask cons.  Every pilot sits at
    least one cell inside the frame (its four neighbours carry the auxiliary
    symbols)."""
    D = fb.fbmc_matrix()
    G = fb.tx_matrix()
    Q = fb.rx_matrix().conj().T
    NP = int(np.sum(pm == 1))
    if method == "Auxiliary":
        aux = pm.copy()
        a, b = np.nonzero(pm.T)
        for r, c in zip(b, a):
            assert 1 <= r < pm.shape[0] - 1 and 1 <= c < pm.shape[1] - 1, (r, c)
            aux[r + 1, c] = -1
            aux[r - 1, c] = -1
            aux[r, c + 1] = -1
            aux[r, c - 1] = -1
        m = osu.iic("Auxiliary", aux, D, 28, P2D_AUX)
        sel = (osu.col(cons) * (osu.col(aux) == 0)) == 1
        cm = np.array([np.sum(np.abs(m["P"][sel, NP + i])) > m["DPR"] * 0.9 for i in range(m["ND"])])
        return dict(G=G, Q=Q, P=m["P"], pilot_pos=np.flatnonzero(osu.col(pm) == 1),
                    data_pos=np.flatnonzero(osu.col(aux) == 0), despread=False, real_detect=True,
                    data_div=float(np.sqrt(m["DPR"])), kappa=float(P2D_AUX * m["DPR"]),
                    symbols=pam[0], bitmap=pam[1].astype(np.uint8), bits_per_symbol=pam[1].shape[1],
                    n_data=m["ND"], considered=cm, bits_slot=0, pilot_slot=0, iic=m)
    assert method == "Coding", method
    m = osu.iic("Coding", pm, D, 20, P2D_COD)
    notcons = osu.col(cons) == 0
    cm = np.array([not np.any(m["P"][notcons, NP + i]) for i in range(m["ND"])])
    return dict(G=G, Q=Q, P=m["P"], pilot_pos=np.flatnonzero(osu.col(pm) == 1),
                data_pos=np.arange(NP, m["P"].shape[1]), despread=True, real_detect=True,
                data_div=float(m["DPR"]), kappa=float(P2D_COD * m["DPR"]), symbols=pam[0],
                bitmap=pam[1].astype(np.uint8), bits_per_symbol=pam[1].shape[1], n_data=m["ND"],
                considered=cm, bits_slot=1, pilot_slot=0, iic=m)


def _mask(L, K, l0, k0):
    cons = np.zeros((L, K))
    cons[l0:L - l0, k0:K - k0] = 1
    return cons


def _lattice(n):
    """n pilots of the default 24 x 14 OFDM frame, drawn without replacement."""
    idx = np.random.default_rng(n).choice(24 * 14, n, replace=False)
    return tuple((int(i % 24), int(i // 24)) for i in idx)


SEED = 0x5EED0002                     # tests/test_gpu_parity.py's


def _ofdm(L, K, srm, zg, pilots, edge=(1, 1), n_rep=16, seed=SEED):
    return SimpleNamespace(kind="ofdm", scheme="ofdm", L=L, K=K, srm=srm, zg=zg, pilots=tuple(pilots), edge=edge,
                           method=None, order=16, n_rep=n_rep, seed=seed)


def _fbmc(L, K, srm, pilots, method, n_rep=16, seed=SEED):
    return SimpleNamespace(kind="fbmc", scheme="fbmc_aux" if method == "Auxiliary" else "fbmc_cod", L=L, K=K, srm=srm,
                           zg=None, pilots=tuple(pilots), edge=(2, 3), method=method, order=4, n_rep=n_rep, seed=seed)


_A = ((1, 1), (7, 1), (4, 3), (10, 5), (2, 5))
_F3 = ((2, 3), (8, 3), (5, 7))
# id -> frame, pilots (l, k) 0-based, constellation order (16-QAM / 4-PAM), realisations 0..n_rep-1 and seed of the
# count check.  The default OFDM frame (24 x 14, N 540) keeps the script's edge mask cons[4:L-4, 5:K-5]; from NP 32
# on its count check takes 8 realisations, from NP 40 on 4 (the oracle's literal D_hat costs LK^2 NP per stage).  fbmc20x9 at the
# suite's seed leaves counters of the 35 dB point at 0 over 16 realisations (4-PAM); at 0x5EED0004 none is.
GEOMETRIES = {
    "ofdm12x7_np5": _ofdm(12, 7, 16, 3, _A),                      # N 125, LK 84 = 3.5 row blocks, ND 79
    "ofdm20x5_np12": _ofdm(20, 5, 24, 5, [(l, k) for k in (0, 2, 4) for l in (0, 6, 12, 19)]),   # N 140, LK 100, ND 88
    "ofdm12x7_np1": _ofdm(12, 7, 16, 3, ((5, 3),)),               # 1 x 1 inverse
    "ofdm24x14_np8": _ofdm(24, 14, 24, 88, _lattice(8), edge=(4, 5)),
    "ofdm24x14_np32": _ofdm(24, 14, 24, 88, _lattice(32), edge=(4, 5), n_rep=8),
    "ofdm24x14_np36": _ofdm(24, 14, 24, 88, _lattice(36), edge=(4, 5), n_rep=8),   # k_rinv's largest in-LDS NP
    "ofdm24x14_np40": _ofdm(24, 14, 24, 88, _lattice(40), edge=(4, 5), n_rep=4),
    "ofdm24x14_np64": _ofdm(24, 14, 24, 88, _lattice(64), edge=(4, 5), n_rep=4),   # DSCE_MAX_NP
    "fbmc12x11_aux_np3": _fbmc(12, 11, 12, _F3, "Auxiliary"),    # N 156, LK 132, ND 117
    "fbmc12x11_cod_np3": _fbmc(12, 11, 12, _F3, "Coding"),       # ND 126
    "fbmc12x11_aux_np8": _fbmc(12, 11, 12, ((2, 2), (5, 3), (8, 2), (2, 5), (5, 6), (8, 5), (3, 8), (7, 8)), "Auxiliary"),
    "fbmc12x15_aux_np16": _fbmc(12, 15, 12, [(l, k) for k in (1, 5, 9, 13) for l in (1, 4, 7, 10)], "Auxiliary"),   # N 180
    "fbmc20x9_aux_np5": _fbmc(20, 9, 24, ((3, 2), (10, 4), (16, 6), (6, 6), (13, 2)), "Auxiliary",
                              seed=0x5EED0004),   # N 288, LK 180
}
OFDM_SMALL = ("ofdm12x7_np5", "ofdm20x5_np12", "ofdm12x7_np1")
OFDM_DEFAULT_FRAME = tuple(g for g in GEOMETRIES if g.startswith("ofdm24x14"))
FBMC = tuple(g for g in GEOMETRIES if g.startswith("fbmc"))


def frame_setup(name, scheme, sc, mod, SR, L, snr_db=SNR, n_iter=2, pdp="VehicularA", velocity_kmh=500.0, paths=20):
    """harness.setup's namespace around one scheme dict sc of modulator mod."""
    pdpv, pdpn, taps = osu.power_delay_profile(SR, pdp)
    fD = velocity_kmh / 3.6 * 2.5e9 / 2.998e8
    chan = dict(N=mod.N, dt=1.0 / SR, pdp=pdpv, pdp_norm=pdpn, idx_taps=taps, fD=fD, paths=int(paths), model="Jakes")
    snr = np.asarray(snr_db, dtype=float)
    pn = SR / (F * L) * 10.0 ** (-snr / 10)
    return SimpleNamespace(name=name, N=mod.N, L=L, SR=SR, snr_db=snr, pn_time=pn, n_iter=n_iter, zero_threshold=1e-8,
                           chan=chan, schemes={scheme: sc}, fbmc=mod if scheme != "ofdm" else None,
                           ofdm=mod if scheme == "ofdm" else None,
                           variant=(int(sc["symbols"].size), str(pdp), float(velocity_kmh), int(paths), "Jakes"))


@functools.lru_cache(maxsize=None)
def geometry_setup(gid, snr_db=SNR):
    """(T, S): GEOMETRIES[gid] and its oracle-format setup (one scheme, SNR
    (15, 35) dB or the tuple snr_db, 2 IC iterations, VehicularA at 500 km/h, 20
    paths); S.name is "geo:" + gid, unique per geometry (harness.oracle_mmse
    caches on it and on the SNR points)."""
    T = GEOMETRIES[gid]
    SR = F * T.srm
    pm = pilot_matrix(T.L, T.K, T.pilots)
    cons = _mask(T.L, T.K, *T.edge)
    if T.kind == "ofdm":
        mod = osu.OFDM(T.L, T.K, F, SR, 0, 1 / 15e3 / 14, T.zg / SR)
        sc = ofdm_scheme(mod, pm, cons, osu.constellation(T.order, "QAM"))
    else:
        mod = osu.FBMC(T.L, T.K, F, SR, 0, 8, 0)
        sc = fbmc_scheme(mod, pm, cons, osu.constellation(T.order, "PAM"), T.method)
    return T, frame_setup("geo:" + gid, T.scheme, sc, mod, SR, T.L, snr_db=snr_db)


def dims(gid):
    """(N, LK, NP, ND) of a geometry."""
    T, S = geometry_setup(gid)
    sc = S.schemes[T.scheme]
    return S.N, sc["G"].shape[1], len(sc["pilot_pos"]), sc["n_data"]


_COUNTS = {}


def oracle_counts(gid):
    """refsim.simulate's result over realisations 0..n_rep-1 of a geometry at its
    seed (once per process; read-only)."""
    if gid not in _COUNTS:
        T, S = geometry_setup(gid)
        _COUNTS[gid] = harness.simulate(S, T.seed, 0, T.n_rep, [T.scheme])
    return _COUNTS[gid]
