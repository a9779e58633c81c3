"""CPU: the script parameters of oracle/setup.py::script_setup (qam_order, pdp,
velocity_kmh, paths, doppler_model) and their way through tests/harness.py.
The defaults are the reference script's point and reproduce the setup the
parity tests have always used; a variant changes the channel and the
constellation and nothing else; harness.oracle_mmse keeps variants apart."""
import numpy as np
import pytest

import harness
from oracle import setup as osu


def _same(a, b, path="setup"):
    """Bit-for-bit equality of two script_setup results (dicts, arrays, scalars;
    the modulator objects by their attributes)."""
    if isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], "%s[%r]" % (path, k))
    elif isinstance(a, (osu.FBMC, osu.OFDM)):
        _same(vars(a), vars(b), path)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, path
        assert np.array_equal(a, b), path
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, "%s[%d]" % (path, i))
    else:
        assert a == b and type(a) is type(b), path


def test_script_setup_defaults_are_the_scripts_point():
    """script_setup() without the new parameters is the script's own point, bit
    for bit: 256-QAM / 16-PAM, VehicularA, 500 km/h at 2.5 GHz, 200 paths,
    'Jakes' — as the explicit call gives, and as the literal expressions the
    function held before it took parameters (the operators G, Q, P and the
    precoders are pinned by tests/golden/setup_*.json, test_oracle.py)."""
    schemes = ("fbmc_aux", "ofdm")
    d = osu.script_setup("default", schemes=schemes, snr_db=[15.0, 35.0])
    e = osu.script_setup("default", schemes=schemes, snr_db=[15.0, 35.0], qam_order=256, pdp="VehicularA",
                         velocity_kmh=500.0, paths=200, doppler_model="Jakes")
    _same(d, e)
    assert d["variant"] == (256, "VehicularA", 500.0, 200, "Jakes")
    ch = d["chan"]
    pdp, pdpn, taps = osu.power_delay_profile(15e3 * 24, "VehicularA")
    assert ch["fD"] == 500 / 3.6 * 2.5e9 / 2.998e8 and ch["paths"] == 200 and type(ch["paths"]) is int
    assert ch["model"] == "Jakes" and ch["N"] == 540 and ch["dt"] == 1.0 / (15e3 * 24)
    assert np.array_equal(ch["pdp"], pdp) and np.array_equal(ch["pdp_norm"], pdpn) and np.array_equal(ch["idx_taps"], taps)
    assert list(taps) == [0, 1]
    qam, pam = osu.constellation(256, "QAM"), osu.constellation(16, "PAM")
    of, fb = d["schemes"]["ofdm"], d["schemes"]["fbmc_aux"]
    assert np.array_equal(of["symbols"], qam[0]) and np.array_equal(of["bitmap"], qam[1].astype(np.uint8))
    assert np.array_equal(fb["symbols"], pam[0]) and np.array_equal(fb["bitmap"], pam[1].astype(np.uint8))
    assert of["bits_per_symbol"] == 8 and fb["bits_per_symbol"] == 4
    # harness.setup: same defaults, same object for the same key
    S = harness.setup("default", schemes=schemes, snr_db=[15.0, 35.0])
    _same(vars(S), d)
    assert harness.setup("default", schemes=schemes, snr_db=[15.0, 35.0], velocity_kmh=500).chan is S.chan


def test_a_variant_changes_channel_and_constellation_only():
    base = harness.setup("default", schemes=("fbmc_aux", "ofdm"), snr_db=[15.0, 35.0])
    var = harness.setup("default", schemes=("fbmc_aux", "ofdm"), snr_db=[15.0, 35.0], qam_order=64, pdp="VehicularB",
                        velocity_kmh=50.0, paths=7, doppler_model="Uniform")
    assert var.variant == (64, "VehicularB", 50.0, 7, "Uniform") and var.variant != base.variant
    ch = var.chan
    assert ch["fD"] == 50.0 / 3.6 * 2.5e9 / 2.998e8 and abs(ch["fD"] * 10 - base.chan["fD"]) < 1e-9
    assert ch["paths"] == 7 and ch["model"] == "Uniform"
    assert list(ch["idx_taps"]) == [0, 3, 5, 6, 7] and ch["pdp"].size == 8 and abs(ch["pdp_norm"].sum() - 1) < 1e-15
    # PAM order = sqrt(QAM order) (script:86-87)
    of, fb = var.schemes["ofdm"], var.schemes["fbmc_aux"]
    assert of["symbols"].size == 64 and of["bits_per_symbol"] == 6 and of["bitmap"].shape == (64, 6)
    assert fb["symbols"].size == 8 and fb["bits_per_symbol"] == 3 and np.all(fb["symbols"].imag == 0)
    for sym in (of["symbols"], fb["symbols"]):
        assert abs(np.mean(np.abs(sym) ** 2) - 1) < 1e-12 and np.unique(sym).size == sym.size
    # everything else is untouched
    for key in ("G", "Q", "P", "pilot_pos", "data_pos", "considered"):
        for name in ("ofdm", "fbmc_aux"):
            assert np.array_equal(var.schemes[name][key], base.schemes[name][key]), (name, key)
    assert np.array_equal(var.pn_time, base.pn_time) and var.N == base.N
    # the other profiles' taps at 360 kHz
    taps = {p: list(harness.setup("default", schemes=("ofdm",), snr_db=[15.0, 35.0], pdp=p).chan["idx_taps"])
            for p in ("Flat", "PedestrianA", "PedestrianB", "VehicularA")}
    assert taps == {"Flat": [0], "PedestrianA": [0], "PedestrianB": [0, 1], "VehicularA": [0, 1]}
    with pytest.raises(ValueError):
        osu.script_setup("default", schemes=("ofdm",), qam_order=32)
    with pytest.raises(ValueError):
        osu.script_setup("default", schemes=("ofdm",), doppler_model="Discrete-Jakes")


def test_oracle_mmse_cache_keeps_variants_apart():
    """Two setups that differ only in a script parameter share name, SNR list,
    n_iter, schemes and threshold; the MMSE cache must still give each its own
    correlation matrices."""
    kw = dict(schemes=("ofdm",), snr_db=[25.0])
    a = harness.setup("default", **kw)
    b = harness.setup("default", pdp="PedestrianA", **kw)
    c = harness.setup("default", velocity_kmh=50.0, **kw)
    ma, mb, mc = (harness.oracle_mmse(S, "ofdm") for S in (a, b, c))
    assert ma is harness.oracle_mmse(harness.setup("default", **kw), "ofdm")       # same point: cached
    assert ma["R_hP"].shape == mb["R_hP"].shape == mc["R_hP"].shape
    scale = np.abs(ma["R_hP"]).max()
    assert np.abs(ma["R_hP"] - mb["R_hP"]).max() > 1e-3 * scale
    assert np.abs(ma["R_hP"] - mc["R_hP"]).max() > 1e-3 * scale
    assert np.abs(mb["R_hP"] - mc["R_hP"]).max() > 1e-3 * scale
    # the constellation does not enter the MMSE build, but has its own entry
    d = harness.setup("default", qam_order=16, **kw)
    md = harness.oracle_mmse(d, "ofdm")
    assert md is not ma and np.array_equal(md["R_hP"], ma["R_hP"])
