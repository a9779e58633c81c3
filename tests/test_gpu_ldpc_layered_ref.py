"""GPU: dsce_ldpc_layered against references that are not its NumPy twin — the
inputs and assertions of tests/test_ldpc_host.py and
tests/test_ldpc_layered_host.py run through the device with make_layers' first-fit
layers: on random cycle-free codes k_ldpc_layered (alpha = 1, no early stop, 4 M +
4 iterations) returns the unique maximum-likelihood codeword found by enumeration
with integer metrics, and on make_ldpc's codes decoding lam0 (1 - 2 c) and XOR-ing
the codeword c of a separate encoder gives the all-zero decode, iteration counts
included, at noise levels where the decoder both fails and succeeds.  A decoder
that never stores R' (the own message is never taken out again) fails the first
(test_ldpc_layered_host.test_wrong_layered_decoders_are_caught); a check rule
with the sign of the other LLR convention, or a butterfly whose minimum leaves out
the wrong lane, fails both.  tests/test_gpu_ldpc_layered.py compares the device
with the twin."""
import pytest

from test_gpu_ldpc_layered import _dec, bare  # noqa: F401  (the fixture)
from test_ldpc_host import TREE_SEEDS, check_invariance, check_tree_ml
from test_ldpc_layered_host import check_invariance_2560_half, layers_of

pytestmark = pytest.mark.gpu


def _layered(eng, lam, code):
    """dsce_ldpc_layered over make_layers(code) (once per code table), its outputs between guard regions"""
    return _dec(eng, lam, code, layers_of(code))


def test_tree_codes_decode_to_the_ml_codeword_on_the_device_layered(bare):  # noqa: F811
    """100 cycle-free codes x 10 integer inputs: 1000 words, each the unique maximiser."""
    assert check_tree_ml(lambda lam, code: _layered(bare, lam, code), TREE_SEEDS) >= 1000


@pytest.mark.parametrize("N,rate", [(96, "1/2"), (96, "3/4"), (96, "5/6"), (2560, "3/4"), (2560, "5/6")])
def test_codeword_invariance_on_the_device_layered(bare, N, rate):  # noqa: F811
    check_invariance(lambda lam, code: _layered(bare, lam, code), N, rate)


def test_codeword_invariance_2560_half_on_the_device_layered(bare):  # noqa: F811
    """(2560, 1/2) at the sigma of the layered schedule's own quarter window."""
    check_invariance_2560_half(lambda lam, code: _layered(bare, lam, code))
