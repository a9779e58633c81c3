"""CPU: the frame geometries of tests/geometries.py are what they claim to be, and
the preconditions of tests/test_gpu_geometries.py hold.  No GPU call.

The builder is the oracle's own restatement, not a second one: fed the script's
pilot matrices it returns script_setup("default")'s scheme dicts array for
array.  Per geometry: the modulator is biorthogonal and the precoder keeps the
frame's power (OFDM), the pilots' signal-to-interference ratio clears the
script's floors (FBMC, script:116-129: 38 dB auxiliary, 28 dB coding), and over
the realisations the GPU test counts the oracle flags no borderline decision,
every counter of the MMSE branch is above zero and cond(R) <= 1e6 (conditions of
an exact comparison and of _check_W's bar, not measurements).  k_rinv's LDS
formula is pinned for every pilot count dsce_add_scheme accepts."""
import os
import re

import numpy as np
import pytest

import harness
import geometries as geo
from oracle import setup as osu

CSRC = os.path.join(harness.PKG, "csrc")


def _same_scheme(got, ref):
    assert set(ref) <= set(got), set(ref) - set(got)
    for key, v in ref.items():
        if key == "iic":
            for k2, v2 in v.items():
                if v2 is not None and not isinstance(v2, dict):
                    np.testing.assert_array_equal(np.asarray(got[key][k2]), np.asarray(v2), err_msg="iic." + k2)
        else:
            np.testing.assert_array_equal(np.asarray(got[key]), np.asarray(v), err_msg=key)
            assert type(got[key]) is type(v) or isinstance(v, np.ndarray), key


def test_builder_restates_script_setup():
    """The script's frame (L 24, 14 OFDM / 30 FBMC symbols, its pilot lattices
    and edge masks, 256-QAM / 16-PAM) through ofdm_scheme and fbmc_scheme:
    script_setup("default")'s ofdm, fbmc_aux and fbmc_cod, every array equal."""
    ref = osu.script_setup("default", snr_db=list(geo.SNR), n_iter=2)
    L, SR = 24, geo.F * 24
    pm_o, pm_f = np.zeros((L, 14)), np.zeros((L, 30))
    for pm, cols, step in ((pm_o, (2, 6, 2, 6), 7), (pm_f, (3, 11, 4, 12), 16)):      # script:91-103 (1-based)
        for r0, c0 in zip((2, 5, 8, 11), cols):
            pm[r0 - 1::12, c0 - 1::step] = 1
    cons_o, cons_f = np.zeros(pm_o.shape), np.zeros(pm_f.shape)
    cons_o[4:L - 4, 5:14 - 5] = 1                                                     # script:145-149
    cons_f[4:L - 4, 10:30 - 10] = 1
    fb = osu.FBMC(L, 30, geo.F, SR, 0, 8, 0)
    of = osu.OFDM(L, 14, geo.F, SR, 0, 1 / 15e3 / 14, 88 / SR)
    assert of.N == fb.N == ref["N"] == 540
    pam, qam = osu.constellation(16, "PAM"), osu.constellation(256, "QAM")
    _same_scheme(geo.ofdm_scheme(of, pm_o, cons_o, qam), ref["schemes"]["ofdm"])
    _same_scheme(geo.fbmc_scheme(fb, pm_f, cons_f, pam, "Auxiliary"), ref["schemes"]["fbmc_aux"])
    _same_scheme(geo.fbmc_scheme(fb, pm_f, cons_f, pam, "Coding"), ref["schemes"]["fbmc_cod"])
    S = geo.frame_setup("x", "ofdm", ref["schemes"]["ofdm"], of, SR, L, paths=200)
    assert set(vars(S)) == set(ref)
    for key in ("N", "L", "SR", "n_iter", "zero_threshold"):
        assert getattr(S, key) == ref[key], key
    np.testing.assert_array_equal(S.pn_time, ref["pn_time"])
    for key, v in ref["chan"].items():
        np.testing.assert_array_equal(np.asarray(S.chan[key]), np.asarray(v), err_msg=key)


DIMS = {   # id: (N, LK, NP, ND)
    "ofdm12x7_np5": (125, 84, 5, 79), "ofdm20x5_np12": (140, 100, 12, 88), "ofdm12x7_np1": (125, 84, 1, 83),
    "ofdm24x14_np8": (540, 336, 8, 328), "ofdm24x14_np32": (540, 336, 32, 304), "ofdm24x14_np36": (540, 336, 36, 300),
    "ofdm24x14_np40": (540, 336, 40, 296), "ofdm24x14_np64": (540, 336, 64, 272),
    "fbmc12x11_aux_np3": (156, 132, 3, 117), "fbmc12x11_cod_np3": (156, 132, 3, 126),
    "fbmc12x11_aux_np8": (156, 132, 8, 92), "fbmc12x15_aux_np16": (180, 180, 16, 100),
    "fbmc20x9_aux_np5": (288, 180, 5, 155),
}


@pytest.mark.parametrize("gid", list(geo.GEOMETRIES))
def test_geometry_is_what_it_claims(gid):
    T, S = geo.geometry_setup(gid)
    sc = S.schemes[T.scheme]
    assert set(geo.GEOMETRIES) == set(DIMS) and geo.dims(gid) == DIMS[gid]
    N, LK, NP, ND = DIMS[gid]
    assert S.name == "geo:" + gid and list(S.schemes) == [T.scheme] and S.n_iter == 2
    assert sc["G"].shape == sc["Q"].shape == (N, LK) and sc["P"].shape == (LK, NP + ND)
    assert len(sc["considered"]) == ND and 0 < np.sum(sc["considered"]) < ND
    assert sc["symbols"].size == T.order and len(set(sc["pilot_pos"])) == NP
    if T.kind == "ofdm":
        # Q'G = I (the cyclic prefix and the guard samples drop out) and the precoder keeps the frame's power
        np.testing.assert_allclose(sc["Q"].conj().T @ sc["G"], np.eye(LK), rtol=0, atol=1e-12)
        assert abs(np.sum(np.abs(sc["P"]) ** 2) - LK) <= 1e-12 * LK
        assert sorted(sc["pilot_pos"]) == sorted(l + T.L * k for l, k in T.pilots)
    else:
        sir = sc["iic"]["SIR_dB"]
        assert sir.shape == (NP,) and sir.min() > (38.0 if T.method == "Auxiliary" else 28.0), sir
        assert not np.imag(sc["symbols"]).any()


def test_geometries_leave_the_scripts_domain():
    """What the table is for: pilot counts off a multiple of 4, NP / 4 outside
    {2, 4, 8}, LK with a partial 24-row block, ND off a multiple of 32, L off
    24 / 48 for FBMC, pilots on the frame's corners."""
    d = DIMS
    assert d["ofdm12x7_np5"][2] % 4 and d["ofdm12x7_np5"][1] % 24 and d["ofdm12x7_np5"][3] % 32
    assert d["ofdm20x5_np12"][2] // 4 == 3 and d["ofdm20x5_np12"][1] % 24
    assert {(0, 0), (19, 0), (0, 4), (19, 4)} <= set(geo.GEOMETRIES["ofdm20x5_np12"].pilots)
    assert 12 % 24 and 20 % 24                               # blocks of 24 rows straddle symbols of 12 / 20
    for g in geo.FBMC:
        assert geo.GEOMETRIES[g].L not in (24, 48) and d[g][1] % 24
    assert sorted(d[g][2] for g in geo.OFDM_DEFAULT_FRAME) == [8, 32, 36, 40, 64]


@pytest.mark.parametrize("gid", list(geo.GEOMETRIES))
def test_preconditions_of_the_gpu_comparison(gid):
    T, S = geo.geometry_setup(gid)
    mm = harness.oracle_mmse(S, T.scheme)
    for key in ("R_est", "R_noI"):
        for k in range(len(S.pn_time)):
            cond = np.linalg.cond(mm[key][k])
            assert cond <= 1e6, (gid, key, k, cond)
    res = geo.oracle_counts(gid)
    assert res["err"].shape == (1, 2, 2, 2, 3)
    assert res["borderline"].sum() == 0, res["borderline"]
    assert res["err"][0, 0].min() > 0, res["err"][0, 0]      # [csi 0 = MMSE][edge][snr][stage]


def test_rinv_lds_formula():
    """k_rinv's in-LDS form takes NP x 3NP x 16 B (kernels_setup.hip): within
    64 KiB up to NP 36, within gfx950's 160 KiB up to NP 58, beyond it from 59.
    The engine uses that form up to 64 KiB and device memory above, and the
    [NP][64] tile of k_ls_hest / k_wcontract_valu is 64 KiB at NP 64, so every
    NP of 1..DSCE_MAX_NP stays within the limit."""
    src = open(os.path.join(CSRC, "kernels_setup.hip")).read()
    hdr = open(os.path.join(CSRC, "dsce_kernels.h")).read()
    assert re.search(r"size_t rinv_lds_bytes\(int NP\) \{ return \(size_t\)NP \* 3 \* NP \* sizeof\(double2\); \}", src)
    assert re.search(r"RINV_LDS_MAX = 64 \* 1024;", hdr) and geo.RINV_LDS_LIMIT == 64 * 1024
    assert re.search(r"hp_tile_lds_bytes\(int NP\) \{ return \(size_t\)NP \* 64 \* sizeof\(double2\); \}", hdr)
    max_np = int(re.search(r"#define DSCE_MAX_NP (\d+)", open(os.path.join(CSRC, "dsce_common.h")).read()).group(1))
    assert max_np == 64
    table = {36: 62208, 37: 65712, 58: 161472, 59: 167088, 64: 196608}
    for n, b in table.items():
        assert geo.rinv_lds_bytes(n) == b
    for n in range(1, max_np + 1):
        b = geo.rinv_lds_bytes(n)
        assert b == 48 * n * n
        assert (b <= 64 * 1024) == (n <= 36) and (b <= 160 * 1024) == (n <= 58)
        assert n * 64 * 16 <= 64 * 1024
