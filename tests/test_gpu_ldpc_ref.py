"""GPU: dsce_ldpc against references that are not its NumPy twin — the inputs and
assertions of tests/test_ldpc_host.py run through the device: on random
cycle-free codes dsce_ldpc (alpha = 1, no early stop) returns the unique
maximum-likelihood codeword found by enumeration with integer metrics, and on
make_ldpc's codes decoding lam0 (1 - 2 c) and XOR-ing the codeword c of a
separate encoder gives the all-zero decode, iteration counts included, at noise
levels where the decoder both fails and succeeds.  A decoder with the check
rule's sign of the other LLR convention, or one that does not exclude the own
message, fails both (test_ldpc_host.test_wrong_decoders_are_caught)."""
import numpy as np
import pytest

from test_gpu_ldpc import _ldpc, bare  # noqa: F401  (the fixture)
from test_ldpc_host import TREE_SEEDS, check_invariance, check_tree_ml

pytestmark = pytest.mark.gpu


def test_tree_codes_decode_to_the_ml_codeword_on_the_device(bare):  # noqa: F811
    """100 cycle-free codes x 10 integer inputs: 1000 words, each the unique maximiser."""
    assert check_tree_ml(lambda lam, code: _ldpc(bare, lam, code), TREE_SEEDS) >= 1000


@pytest.mark.parametrize("rate", ["1/2", "3/4", "5/6"])
@pytest.mark.parametrize("N", [96, 2560])
def test_codeword_invariance_on_the_device(bare, N, rate):  # noqa: F811
    from dsce.coding import ldpc_decode
    from test_ldpc_host import INVARIANCE_SIGMA, bpsk_lam0, code_of
    check_invariance(lambda lam, code: _ldpc(bare, lam, code), N, rate)
    # and the device's all-zero decode is the twin's
    code = code_of(N, rate)
    lam0, _ = bpsk_lam0(code, INVARIANCE_SIGMA[N, rate], 40, 1000 + N)
    x, it = _ldpc(bare, lam0, code)
    rx, rit = ldpc_decode(lam0, code)
    assert np.array_equal(x, rx) and np.array_equal(it, rit)
