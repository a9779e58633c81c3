"""Host side of the coded-link track (include/dsce.h, DSCE_HAS_CODED_RUN): the
rate-1/2, constraint-length-7 convolutional code (133, 171 octal), the code
tables that carry interleaving and puncturing, and viterbi_decode, the NumPy
twin of the engine's k_viterbi: the same fp64 operations in the same order, so
its decisions equal the engine's to the bit.

State s holds u_{t-1} in bit 0 .. u_{t-6} in bit 5; next state ns = ((s << 1) |
u_t) & 63; the predecessors of ns are p_b = (ns >> 1) | (b << 5), b = 0, 1, with
input u_t = ns & 1.  The register r = (p_b << 1) | u_t = ns | (b << 6) holds
u_t .. u_{t-6} in bits 0 .. 6, and output k is the parity of r & TAPS[k].
"""
from __future__ import annotations

import collections

import numpy as np

K_LEN = 7                     # constraint length
N_STATES = 64
N_TAIL = K_LEN - 1            # tail zeros of a terminated codeword
MAX_STEPS = 8192              # dsce_run_coded / dsce_viterbi: the decision words of a codeword stay within 64 KiB
# bit d of TAPS[k]: u_{t-d} enters output k.  o0: 0, 2, 3, 5, 6 (133 octal); o1: 0, 1, 2, 3, 6 (171 octal)
TAPS = (0b1101101, 0b1001111)
# (keep o0, keep o1) per trellis step, repeating
PUNCTURE = {
    "1/2": ((1, 1),),
    "2/3": ((1, 1), (1, 0)),
    "3/4": ((1, 1), (1, 0), (0, 1)),
    "5/6": ((1, 1), (1, 0), (0, 1), (1, 0), (0, 1)),
}

Code = collections.namedtuple("Code", "src terminated n_slots rate n_steps n_info n_kept")
Code.__doc__ = """A code table for dsce_run_coded / dsce_viterbi: src int32 [n_steps][2], the slot
that carries output k of step t or -1 for a punctured one; n_info = n_steps - 6 if
terminated (the last six inputs are tail zeros) else n_steps; n_kept outputs are
transmitted in n_slots slots."""


def _parity(v):
    v = np.asarray(v)
    p = np.zeros(v.shape, dtype=np.uint8)
    for d in range(K_LEN):
        p ^= ((v >> d) & 1).astype(np.uint8)
    return p


def conv_encode(u):
    """The coded bits of the input sequences u [..][T] (0 / 1): uint8 [..][T][2],
    o0 = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6} and o1 = u_t ^ u_{t-1} ^ u_{t-2} ^
    u_{t-3} ^ u_{t-6} with u_t = 0 for t < 0.  Nothing is appended: a terminated
    codeword is one whose last six inputs are 0."""
    u = np.asarray(u).astype(np.uint8) & 1
    T = u.shape[-1]
    pad = np.concatenate([np.zeros(u.shape[:-1] + (N_TAIL,), dtype=np.uint8), u], axis=-1)
    out = np.zeros(u.shape + (2,), dtype=np.uint8)
    for k in range(2):
        for d in range(K_LEN):
            if (TAPS[k] >> d) & 1:
                out[..., k] ^= pad[..., N_TAIL - d:N_TAIL - d + T]
    return out


def info_bits(n_steps, terminated):
    return int(n_steps) - N_TAIL if terminated else int(n_steps)


def make_code(n_slots, rate="1/2", terminated=True, interleaver=7):
    """The code table of `rate` ('1/2', '2/3', '3/4', '5/6': the puncturing masks of
    PUNCTURE) for n_slots coded-bit slots: n_steps is the largest step count
    whose kept outputs number at most n_slots, and the q-th kept output, in (t, k)
    order, goes to slot pi[q].  interleaver: an int seed (pi =
    numpy.random.RandomState(seed).permutation(n_slots), a frozen stream), an
    explicit permutation of range(n_slots), or None for the identity."""
    if rate not in PUNCTURE:
        raise ValueError("rate must be one of %s" % sorted(PUNCTURE))
    mask = PUNCTURE[rate]
    n_slots = int(n_slots)
    per = sum(a + b for a, b in mask)
    T = (n_slots // per) * len(mask)
    kept = (n_slots // per) * per
    while kept + sum(mask[T % len(mask)]) <= n_slots:
        kept += sum(mask[T % len(mask)])
        T += 1
    if T < 1 or (terminated and T < K_LEN) or T > MAX_STEPS:
        raise ValueError("%d slots at rate %s give %d trellis steps (1 .. %d, at least %d terminated)"
                         % (n_slots, rate, T, MAX_STEPS, K_LEN))
    if interleaver is None:
        pi = np.arange(n_slots)
    elif isinstance(interleaver, (int, np.integer)):
        pi = np.random.RandomState(int(interleaver)).permutation(n_slots)
    else:
        pi = np.asarray(interleaver, dtype=np.int64).reshape(-1)
        if pi.size != n_slots or not np.array_equal(np.sort(pi), np.arange(n_slots)):
            raise ValueError("interleaver must be a permutation of range(n_slots)")
    keep = np.array([mask[t % len(mask)] for t in range(T)], dtype=bool)          # [T][2]
    src = np.full((T, 2), -1, dtype=np.int32)
    src[keep] = pi[:kept]
    return Code(src=src, terminated=bool(terminated), n_slots=n_slots, rate=rate, n_steps=T,
                n_info=info_bits(T, terminated), n_kept=kept)


def code_lam(coded, src, n_slots, amplitude=1.0):
    """The noiseless decoder input of the codewords coded [..][T][2] under table
    src: lam [..][n_slots] = +amplitude where the slot carries a 1, -amplitude
    for a 0, and 0 in the slots the table does not use."""
    coded = np.asarray(coded)
    src = np.asarray(src)
    lam = np.zeros(coded.shape[:-2] + (int(n_slots),))
    use = src >= 0
    lam[..., src[use]] = amplitude * (2.0 * coded[..., use].astype(np.float64) - 1.0)
    return lam


def viterbi_decode(lam, src, terminated):
    """Maximum-likelihood sequence decoding of lam [n_cw][n_slots] (or [n_slots];
    positive = the bit is 1) under table src [T][2]: uint8 [n_cw][T] decoded inputs.
    The twin of k_viterbi, in fp64 and in its order: pm[0] = 0, pm[s] = -inf
    otherwise; per step z_k = lam[src[t][k]] (0.0 for -1), c_b = (pm[p_b] + (o0 ? z_0
    : 0.0)) + (o1 ? z_1 : 0.0), decision d = c_1 > c_0 (a tie takes b = 0), pm[ns]
    = d ? c_1 : c_0 without renormalisation; traceback from state 0 if terminated,
    else from the largest pm (lowest index on ties); u_t is bit 0 of the state
    after step t."""
    lam = np.asarray(lam, dtype=np.float64)
    single = lam.ndim == 1
    lam = np.ascontiguousarray(lam.reshape(-1, lam.shape[-1]))
    src = np.asarray(src, dtype=np.int64).reshape(-1, 2)
    T, n = src.shape[0], lam.shape[0]
    ns = np.arange(N_STATES)
    pred = np.stack([ns >> 1, (ns >> 1) | 32])                                   # [b][ns]
    reg = np.stack([ns, ns | 64])
    o = np.stack([_parity(reg & TAPS[0]), _parity(reg & TAPS[1])]).astype(bool)  # [k][b][ns]
    pm = np.full((n, N_STATES), -np.inf)
    pm[:, 0] = 0.0
    dec = np.zeros((T, n, N_STATES), dtype=bool)
    zero = np.zeros((n, 1))
    with np.errstate(invalid="ignore"):
        for t in range(T):
            z = [lam[:, src[t, k]][:, None] if src[t, k] >= 0 else zero for k in range(2)]
            c = [(pm[:, pred[b]] + np.where(o[0, b], z[0], 0.0)) + np.where(o[1, b], z[1], 0.0) for b in range(2)]
            d = c[1] > c[0]
            dec[t] = d
            pm = np.where(d, c[1], c[0])
    state = np.zeros(n, dtype=np.int64) if terminated else np.argmax(pm, axis=1)
    out = np.zeros((n, T), dtype=np.uint8)
    rows = np.arange(n)
    for t in range(T - 1, -1, -1):
        out[:, t] = state & 1
        state = (state >> 1) | (dec[t, rows, state].astype(np.int64) << 5)
    return out[0] if single else out


def count_errors(decoded, terminated):
    """bit_err, frame_err per codeword of decoded [..][T] inputs of the all-zero
    information word: the ones among the first n_info inputs, and whether any."""
    decoded = np.asarray(decoded)
    k = info_bits(decoded.shape[-1], terminated)
    bit = decoded[..., :k].astype(np.int64).sum(axis=-1)
    return bit, (bit > 0).astype(np.int64)


def coded_counts(llr, sym, code):
    """The definition of dsce_run_coded on exported arrays: llr [n][n_snr][S][ND][m]
    (export_llr) and sym [n][ND] (export) -> dict(bit_err, frame_err), int64
    [n_snr][S].  lam_i = t_i ? -LLR_i : LLR_i with t_i = bit b of sym[rep][j] for
    slot i = j m + b; the decoded inputs of the all-zero information word are
    counted."""
    llr = np.asarray(llr, dtype=np.float64)
    n, nk, S, nd, m = llr.shape
    t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(n, 1, 1, nd * m)
    flat = llr.reshape(n, nk, S, nd * m)
    lam = np.where(t, -flat, flat)
    dec = viterbi_decode(lam.reshape(n * nk * S, nd * m), code.src, code.terminated)
    bit, frame = count_errors(dec, code.terminated)
    return dict(bit_err=bit.reshape(n, nk, S).sum(axis=0), frame_err=frame.reshape(n, nk, S).sum(axis=0))
