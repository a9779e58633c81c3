"""GPU: the three bulk exports on one context.  They share the context's
staging buffer (grown when a call needs more, reused otherwise) and the walk
over sub-batches; every other export test uses one kind per handle.  Here one
handle runs, with host destinations, 70 realisations from first_rep 5 at batch
64 (two sub-batches, the second ragged): export(xp), export_llr, export_stages,
export (all fields), export(xp) again.  Bytes staged per realisation at this
setup (2 SNR points, 2 stages, 256-QAM): 256, 112640, 54272, 28928, 256, so the
buffer grows for the second call and is reused, larger than needed, by the
rest.  Each result must equal the same call on a fresh context, bit for bit
(NaN = "formed by no kernel of the path" equal to NaN), and dsce_run's counts on
the shared context afterwards those of a fresh one."""
import numpy as np
import pytest

import harness
from test_gpu_export import SEED, SNR

pytestmark = pytest.mark.gpu

FIRST, NREP = 5, 70
CALLS = (
    ("export", dict(fields=("xp",))),
    ("export_llr", {}),
    ("export_stages", {}),
    ("export", {}),
    ("export", dict(fields=("xp",))),
)


def _equal(a, b, tag):
    assert sorted(a) == sorted(b), tag
    for f in a:
        assert a[f].dtype == b[f].dtype and a[f].shape == b[f].shape, (tag, f)
        if f.startswith("dec_"):
            assert np.array_equal(a[f], b[f]), (tag, f)          # -1 stays -1
        else:
            assert np.array_equal(a[f], b[f], equal_nan=True), (tag, f)


def test_exports_share_one_context():
    S = harness.setup("default", schemes=("ofdm",), snr_db=SNR, n_iter=1)
    shared = harness.engine(S, batch=64)
    try:
        got = [getattr(shared, name)(0, SEED, FIRST, NREP, **kw) for name, kw in CALLS]
        counts = shared.run(SEED, FIRST, NREP)
    finally:
        shared.close()
    for i, (name, kw) in enumerate(CALLS):
        fresh = harness.engine(S, batch=64)
        try:
            ref = getattr(fresh, name)(0, SEED, FIRST, NREP, **kw)
        finally:
            fresh.close()
        assert all(v.shape[0] == NREP for v in ref.values())
        _equal(got[i], ref, "call %d: %s%s" % (i, name, kw or ""))
    fresh = harness.engine(S, batch=64)
    try:
        ref_counts = fresh.run(SEED, FIRST, NREP)
    finally:
        fresh.close()
    assert counts.sum() > 0 and np.array_equal(counts, ref_counts)
