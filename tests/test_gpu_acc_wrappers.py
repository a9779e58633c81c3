"""GPU: the `out` handling that Engine.run_soft, run_calib, run_coded and run_ldpc
share — what each refuses before the engine is called (an unknown key, a wrong
dtype, a non-contiguous view, a wrong shape, each with its ValueError text), that
the engine returns its reference result afterwards, and the keys of the default
`out`.  Default setup, OFDM, SNR (10, 35), n_iter 4, batch 64, realisations 5..7."""
import numpy as np
import pytest

import harness
from test_gpu_export import SEED, SNR

pytestmark = pytest.mark.gpu

# wrapper -> (noun of its messages, dtype of its arrays, every key, the keys of a default out with branch "perfect")
WRAPPERS = {
    "run_soft": ("soft", np.float64, ["loss_est", "loss_perf0"], ["loss_est"]),
    "run_calib": ("calibration", np.float64, ["ratio_est", "ratio_perf0"], ["ratio_est"]),
    "run_coded": ("coded", np.int64, ["bit_err", "frame_err"], ["bit_err", "frame_err"]),
    "run_ldpc": ("ldpc", np.int64, ["bit_err", "frame_err", "iter_sum"], ["bit_err", "frame_err", "iter_sum"]),
}


@pytest.fixture(scope="module")
def acc_ofdm():
    from dsce.coding import make_code, make_ldpc
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=4)
    eng = harness.engine(S, batch=64)
    sc = S.schemes["ofdm"]
    B = sc["n_data"] * sc["bits_per_symbol"]
    small = make_ldpc(200, "1/2", max_iter=12)
    small = small._replace(slot=np.random.default_rng(4).permutation(B)[:200].astype(np.int32), n_slots=B)
    yield eng, {"run_coded": make_code(B, "3/4", interleaver=7), "run_ldpc": small}
    eng.close()


@pytest.mark.parametrize("name", list(WRAPPERS))
def test_out_of_the_accumulating_wrappers(acc_ofdm, name):
    eng, codes = acc_ofdm
    noun, dtype, keys, perfect_keys = WRAPPERS[name]
    shapes = getattr(eng, {"run_soft": "soft_shapes", "run_calib": "calib_shapes", "run_coded": "coded_shapes",
                           "run_ldpc": "ldpc_shapes"}[name])(0)
    assert list(shapes) == keys
    extra = (codes[name],) if name in codes else ()

    def call(**k):
        return getattr(eng, name)(0, SEED, 5, 3, *extra, **k)

    ref = call()
    assert list(ref) == keys                                                    # the default out: every key ...
    assert list(call(branch="perfect")) == perfect_keys                         # ... but perf0 with the perfect branch
    for f in keys:
        assert ref[f].dtype == dtype and ref[f].shape == shapes[f] and ref[f].flags.c_contiguous, f
    assert sum(int((ref[f] != 0).sum()) for f in keys) > 0

    def refused(out, text):
        before = {f: a.copy() for f, a in out.items() if isinstance(a, np.ndarray)}
        with pytest.raises(ValueError) as e:
            call(out=out)
        assert str(e.value) == text
        for f, a in before.items():
            assert np.array_equal(out[f], a), f                                 # nothing was added
        again = call()                                                          # the engine still works
        assert list(again) == keys
        for f in keys:
            assert np.array_equal(again[f], ref[f]), f

    f = keys[0]
    shp = shapes[f]
    must = "%s must be a C-contiguous %s array of shape %s" % (f, np.dtype(dtype).name, shp)
    refused({f: np.zeros(shp, dtype=dtype), "nothing": np.zeros(shp, dtype=dtype)},
            "unknown %s output 'nothing' (of %s)" % (noun, keys))
    refused({f: np.zeros(shp, dtype=np.float32)}, must)
    refused({f: np.zeros(shp, dtype=np.int32)}, must)
    refused({f: np.zeros(shp + (2,), dtype=dtype)[..., 0]}, must)               # the shape, but strided
    refused({f: np.zeros(shp[:-1] + (shp[-1] + 1,), dtype=dtype)}, must)
    refused({f: np.zeros(shp, dtype=dtype).tolist()}, must)                     # not an array
    # a given out is returned itself, with the sums added into its arrays
    mine = {f: ref[f].copy()}
    got = call(out=mine)
    assert got is mine and list(got) == [f]
    if dtype == np.int64:
        assert np.array_equal(got[f], 2 * ref[f])
    else:
        np.testing.assert_allclose(got[f], 2 * ref[f], rtol=1e-14, atol=0)
