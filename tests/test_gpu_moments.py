"""GPU: the device against itself, by Monte Carlo.  The engine states the channel
twice: the analytic side (k_time_correlation -> k_mcoef -> k_rhp / k_rest_diag /
k_rdij -> k_rinv -> k_w; dsce_get_correlation, dsce_get_W) sees no random number,
and the Monte-Carlo side (the Philox streams -> the Jakes kernels -> TX and
receiver front -> k_export; dsce_export) never reads the J0 table.  Here the
second moments of the second are held against the first (tests/moments.py):

  a   E{h_i conj(h_j)} at the pilots            against R_hP
  b   E{h_c conj(h_p)}, every c and pilot p     against the rows (c, c) of R_Dij = W_cc R_est[k]
  c   E|hp_ls_i|^2 per SNR point                against diag R_est[k]
  d   E{(h_est_c - h_c) conj(hp_ls_j)}          against 0, with the device's own h_est (k_export's stage 0), and the
                                                off-diagonal of E{hp_ls hp_ls^H} against R_est[k]

every entry within moments.BAR = 6 standard errors (the derivation is in
tests/moments.py; seeds are fixed).  a, b and c are asserted for every case, d for
the OFDM cases; for FBMC, whose auxiliary and spread symbols depend on the pilots,
d is not exact in expectation: it is computed and printed.  The oracle supplies
only the setup arrays, as everywhere; no oracle result is compared.  What this
cannot see is an error that both device sides share by construction (a wrong G,
Q or P handed to both); tests/test_moments_host.py proves the statistic and its
power (an fD off by 7 % is caught at 2048 realisations, so 1.2 % at 65536).

tools/moments_measure.py runs the same cases and records times, n and max z per
family in profiles/moments_measure.json."""
import time

import numpy as np
import pytest

import harness
import moments
from test_moments_host import setup_of

pytestmark = pytest.mark.gpu

SEED = 0x5EED0012
SNR = (0.0, 20.0, 40.0)
CHUNK = 4096
N = 65536
# case -> (scheme, keyword arguments of harness.setup beyond "default", or a geometry of tests/geometries.py).  The
# default frame (24 x 14, N 540, 0.93 ms) at 500 km/h spans 1.7 periods of fD: J0 swings through two zeros.
CASES = {
    "default": ("ofdm", {}),
    "uniform": ("ofdm", dict(doppler_model="Uniform")),              # the sinc table
    "paths1": ("ofdm", dict(paths=1)),                               # 1 / sqrt(paths); samples far from Gaussian
    "static": ("ofdm", dict(velocity_kmh=0.0)),                      # the static branch: correlation 1
    "vehicularB": ("ofdm", dict(pdp="VehicularB")),                  # delays far beyond tap 2
    "pedestrianA": ("ofdm", dict(pdp="PedestrianA")),
    "fbmc_aux": ("fbmc_aux", {}),
    "fbmc_cod": ("fbmc_cod", {}),
    "np36": ("ofdm", "ofdm24x14_np36"),                              # k_rinv at its largest in-LDS size, through W_cc
}
# realisations per case: N halved until the case takes a few seconds on one MI355X
N_OF = {c: N for c in CASES}


def case_setup(case):
    scheme, how = CASES[case]
    if isinstance(how, str):
        return scheme, setup_of(how, SNR)[1]
    return scheme, harness.setup("default", schemes=(scheme,), snr_db=SNR, **how)


def measure(case, n=None, chunk=CHUNK, setup=None):
    """Runs one case: dict(n, scheme, z = family -> max z, at = family -> index, seconds = setup / export /
    host).  With setup = (scheme, S) the case's samples, taken with that setup's estimator, are held against that
    setup's analytic side (the negative control)."""
    n = N_OF[case] if n is None else n
    scheme, S = case_setup(case)
    wrong = None if setup is None else harness.engine(setup[1], batch=64)
    sc = S.schemes[scheme]
    pp, ns = np.asarray(sc["pilot_pos"]), len(S.pn_time)
    t0 = time.perf_counter()
    eng = harness.engine(S, batch=chunk)
    try:
        d = eng.scheme_dims(0)
        LK, NP = d.lk, d.n_pilots
        side = wrong or eng
        R_hP, R_est, _ = side.correlation(0)
        W_cc = [moments.diag_rows(side.W(0, k, 0), LK, NP) for k in range(ns)]
        t1 = time.perf_counter()
        fam = moments.Families(LK, pp, ns)
        t_exp = t_host = 0.0
        for first in range(0, n, chunk):
            ta = time.perf_counter()
            e = eng.export(0, SEED, first, min(chunk, n - first), fields=("h", "hp_ls", "h_est"))
            tb = time.perf_counter()
            h_est = e["h_est"] if wrong is None else np.einsum("kcp,nkp->nkc", np.stack(W_cc), e["hp_ls"])
            fam.add(e["h"], e["hp_ls"], h_est)
            t_exp += tb - ta
            t_host += time.perf_counter() - tb
    finally:
        eng.close()
        if wrong is not None:
            wrong.close()
    assert fam.n == n and LK == sc["G"].shape[1] and NP == pp.size
    # R_Dij's rows (c, c) from the device's own W and R_est: one per SNR point, all the same matrix up to W's
    # entries below the zero threshold (at most NP of them per row, each times an entry of R_est)
    R_Dij_cc = [W_cc[k] @ R_est[k] for k in range(ns)]
    atol = 2 * NP * S.zero_threshold * np.abs(R_est).max() + 1e-9 * np.abs(R_Dij_cc[0]).max()
    for k in range(1, ns):
        np.testing.assert_allclose(R_Dij_cc[k], R_Dij_cc[0], rtol=0, atol=atol, err_msg="W R_est, SNR %d" % k)
    sco = fam.scores(R_hP, R_Dij_cc[0], R_est)
    out = dict(case=case, scheme=scheme, n=n, lk=LK, n_pilots=NP, z={f: round(v[0], 3) for f, v in sco.items()},
               at={f: list(v[1]) for f, v in sco.items()},
               seconds=dict(setup=round(t1 - t0, 3), export=round(t_exp, 3), host=round(t_host, 3)))
    print("moments %s" % out)
    return out


@pytest.mark.parametrize("case", list(CASES))
def test_moments_of_the_export_are_the_analytic_side(case):
    r = measure(case)
    asserted = ("a", "b", "c") + (("off", "d") if r["scheme"] == "ofdm" else ())
    for f in asserted:
        assert r["z"][f] <= moments.BAR, (case, f, r["z"][f], r["at"][f])
    # a case that is trivially met checks nothing: the samples spread
    assert all(np.isfinite(r["z"][f]) for f in r["z"])


def test_a_velocity_off_by_three_percent_is_caught():
    """The negative control at the device's n: the default case's samples against the analytic side of an engine
    set up for 515 km/h fail a, b, the off-diagonal and, with that engine's W on the exported LS estimates, d; c, the
    powers, does not depend on fD and stays under the bar.  tests/test_moments_host.py derives 1.2 % as the
    smallest factor caught at this n, so 3 % leaves a factor of two."""
    r = measure("default", setup=("ofdm", harness.setup("default", schemes=("ofdm",), snr_db=SNR, velocity_kmh=515.0)))
    for f in ("a", "b", "off", "d"):
        assert r["z"][f] > moments.BAR, (f, r["z"][f])
    assert r["z"]["c"] <= moments.BAR, r["z"]["c"]


def test_cases_differ_on_the_analytic_side():
    """The cases are different physics, not one matrix five times: R_hP of the default case differs from that of
    every other OFDM case on the default pilots by far more than a standard error at N realisations (1 / 256 of the
    diagonal)."""
    def rhp(case):
        scheme, S = case_setup(case)
        eng = harness.engine(S, batch=64)
        try:
            return eng.correlation(0)[0]
        finally:
            eng.close()

    base = rhp("default")
    for case in ("uniform", "static", "vehicularB", "pedestrianA"):
        other = rhp(case)
        assert np.abs(other - base).max() > 10 * base[0, 0].real / np.sqrt(N), case
