"""Host side of the coded-link track (include/dsce.h, DSCE_HAS_CODED_RUN): the
rate-1/2, constraint-length-7 convolutional code (133, 171 octal), the code
tables that carry interleaving and puncturing, and viterbi_decode, the NumPy
twin of the engine's k_viterbi: the same fp64 operations in the same order, so
its decisions equal the engine's to the bit.  Below it the LDPC side
(DSCE_HAS_LDPC_RUN): make_ldpc's systematic repeat-accumulate codes, their
encoder, and ldpc_decode, the NumPy twin of k_ldpc.

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


# ---- LDPC codes and the normalised min-sum decoder (include/dsce.h, DSCE_HAS_LDPC_RUN) ----

LDPC_MAX_CHECK_DEGREE = 32
LDPC_MAX_ITER = 100
LDPC_RATES = {"1/2": (1, 2), "2/3": (2, 3), "3/4": (3, 4), "5/6": (5, 6)}

LdpcCode = collections.namedtuple(
    "LdpcCode", "row_ptr col slot n_vars n_checks n_info max_iter alpha early_stop n_slots rate four_cycles")
LdpcCode.__doc__ = """An LDPC code for dsce_run_ldpc / dsce_ldpc: H by check in CSR form (row_ptr int32
[n_checks + 1], col int32 [E], the variables of a check strictly ascending), slot int32
[n_vars] (the slot that carries a variable, -1: punctured), variables 0 .. n_info - 1 the
information bits, and the decoder's parameters.  four_cycles: the 4-cycles left in H
(make_ldpc; None for a hand-made code)."""


def ldpc_from_rows(rows, n_vars, n_info, slot=None, n_slots=None, max_iter=30, alpha=0.75, early_stop=True,
                   rate=None, four_cycles=None):
    """An LdpcCode from the variable lists of its checks (each sorted here)."""
    rows = [sorted(int(v) for v in r) for r in rows]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = np.array([v for r in rows for v in r], dtype=np.int32)
    slot = np.arange(n_vars, dtype=np.int32) if slot is None else np.asarray(slot, dtype=np.int32)
    if n_slots is None:
        n_slots = int(slot.max()) + 1 if slot.size and slot.max() >= 0 else 0
    return LdpcCode(row_ptr, col, slot, int(n_vars), len(rows), int(n_info), int(max_iter), float(alpha),
                    bool(early_stop), int(n_slots), rate, four_cycles)


def ldpc_four_cycles(code):
    """The number of 4-cycles of H: sum over pairs of checks of C(common variables, 2)."""
    H = np.zeros((code.n_checks, code.n_vars), dtype=np.float32)
    H[np.repeat(np.arange(code.n_checks), np.diff(code.row_ptr)), code.col] = 1.0
    G = np.rint(H @ H.T).astype(np.int64)
    G = np.triu(G, 1)
    return int((G * (G - 1) // 2).sum())


def make_ldpc(n_slots, rate="1/2", seed=7, interleaver=7, max_iter=30, alpha=0.75, early_stop=True):
    """A systematic repeat-accumulate code H = [H1 | H2] of N = n_slots variables for
    `rate` ('1/2', '2/3', '3/4', '5/6'): K = n_slots * num // den information bits
    (variables 0 .. K - 1) and M = N - K checks.  H2 is the M x M dual diagonal:
    check i holds parity variables K + i and, for i > 0, K + i - 1.  H1 has column
    weight 3 and row weights equal to within one: column after column, each of its
    three rows is drawn from the rows of least weight, among them one that closes no
    4-cycle with the columns placed so far or with H2 where there is one; four_cycles
    reports those that remain.  Every draw comes from numpy.random.RandomState(seed),
    a frozen stream.  Variable v travels in slot pi[v]: interleaver as for make_code
    (an int seed, a permutation, or None for the identity)."""
    if rate not in LDPC_RATES:
        raise ValueError("rate must be one of %s" % sorted(LDPC_RATES))
    num, den = LDPC_RATES[rate]
    N = int(n_slots)
    K = N * num // den
    M = N - K
    if K < 1 or M < 3:
        raise ValueError("%d slots at rate %s give %d information bits and %d checks (at least 1 and 3)"
                         % (N, rate, K, M))
    if (3 * K + M - 1) // M + 2 > LDPC_MAX_CHECK_DEGREE:
        raise ValueError("check degree above %d" % LDPC_MAX_CHECK_DEGREE)
    rng = np.random.RandomState(int(seed))
    weight = np.zeros(M, dtype=np.int64)
    paired = np.zeros((M, M), dtype=bool)                 # rows that already share a column
    idx = np.arange(M - 1)
    paired[idx, idx + 1] = paired[idx + 1, idx] = True     # H2: column K + i joins checks i and i + 1
    rows = [[] for _ in range(M)]
    for j in range(K):
        chosen = []
        for _ in range(3):
            free = np.ones(M, dtype=bool)
            free[chosen] = False
            cand = np.flatnonzero(free & (weight == weight[free].min()))
            cand = cand[rng.permutation(cand.size)]
            clean = cand[~paired[np.ix_(cand, chosen)].any(axis=1)] if chosen else cand
            chosen.append(int(clean[0] if clean.size else cand[0]))
            weight[chosen[-1]] += 1
        for a in chosen:
            rows[a].append(j)
            for b in chosen:
                if a != b:
                    paired[a, b] = True
    for i in range(M):
        rows[i] += [K + i - 1, K + i] if i else [K]
    if interleaver is None:
        pi = np.arange(N)
    elif isinstance(interleaver, (int, np.integer)):
        pi = np.random.RandomState(int(interleaver)).permutation(N)
    else:
        pi = np.asarray(interleaver, dtype=np.int64).reshape(-1)
        if pi.size != N or not np.array_equal(np.sort(pi), np.arange(N)):
            raise ValueError("interleaver must be a permutation of range(n_slots)")
    code = ldpc_from_rows(rows, N, K, slot=pi, n_slots=N, max_iter=max_iter, alpha=alpha, early_stop=early_stop,
                          rate=rate)
    return code._replace(four_cycles=ldpc_four_cycles(code))


def ldpc_encode(u, code):
    """The codewords [..][n_vars] (uint8) of the information words u [..][n_info] under a
    make_ldpc code: the parity bits are the prefix XOR of H1 u, p_i = p_{i-1} ^ (H1 u)_i."""
    u = np.asarray(u).astype(np.uint8) & 1
    K, M = code.n_info, code.n_checks
    if u.shape[-1] != K or code.n_vars != K + M:
        raise ValueError("u must be [..][n_info] of a systematic code with n_vars = n_info + n_checks")
    chk = np.repeat(np.arange(M), np.diff(code.row_ptr))
    info = code.col < K
    s = np.zeros(u.shape[:-1] + (M,), dtype=np.uint8)
    np.bitwise_xor.at(s, (Ellipsis, chk[info]), u[..., code.col[info]])
    return np.concatenate([u, np.bitwise_xor.accumulate(s, axis=-1)], axis=-1)


def ldpc_lam(cw, code, amplitude=1.0):
    """The noiseless decoder input of the codewords cw [..][n_vars]: lam [..][n_slots] =
    +amplitude where the slot carries a 1, -amplitude for a 0, 0 in unused slots."""
    cw = np.asarray(cw)
    lam = np.zeros(cw.shape[:-1] + (code.n_slots,))
    use = code.slot >= 0
    lam[..., code.slot[use]] = amplitude * (2.0 * cw[..., use].astype(np.float64) - 1.0)
    return lam


def ldpc_syndrome(x, code):
    """H x [..][n_checks] (uint8) of the words x [..][n_vars]."""
    x = np.asarray(x).astype(np.uint8) & 1
    return np.bitwise_xor.reduceat(x[..., code.col], code.row_ptr[:-1], axis=-1)


def ldpc_decode(lam, code, _mutate=None):
    """Normalised min-sum decoding of lam [n_cw][n_slots] (or [n_slots]; positive = the
    bit is 1) under `code`: (x uint8 [n_cw][n_vars], it int32 [n_cw]), the decided bits
    of the last iteration performed and the number of iterations.  The twin of k_ldpc,
    in fp64 and in the order of include/dsce.h: ell_v = -lam[slot[v]] (0.0 for -1), P =
    ell, R = 0; per iteration and check, over the edge positions p in order, q_p = P_v -
    R_p, a_p = |q_p|, s_p = q_p < 0, m1 / i1 the minimum and the lowest position
    attaining it, m2 the minimum of the others, sg the XOR of the s_p, R'_p = +-(alpha
    * (p == i1 ? m2 : m1)), negative where sg ^ s_p; per variable P' = ((ell + R'_e1) +
    R'_e2) + .. over its edges in ascending check order; x = P' < 0; with early_stop a
    codeword stops once H x = 0.  _mutate is for the tests only: a deliberately wrong
    decoder ('sign', 'no_exclude', 'alpha_late')."""
    lam = np.asarray(lam, dtype=np.float64)
    single = lam.ndim == 1
    lam = np.ascontiguousarray(lam.reshape(-1, lam.shape[-1]))
    n, N, M = lam.shape[0], code.n_vars, code.n_checks
    row_ptr = np.asarray(code.row_ptr, dtype=np.int64)
    col = np.asarray(code.col, dtype=np.int64)
    slot = np.asarray(code.slot, dtype=np.int64)
    alpha = float(code.alpha)
    deg = np.diff(row_ptr)
    E = col.size
    chk = np.repeat(np.arange(M), deg)
    pos = np.arange(E) - row_ptr[chk]
    by_var = np.argsort(col, kind="stable")                 # a variable's edges in ascending check order
    vdeg = np.bincount(col, minlength=N)
    vptr = np.concatenate([[0], np.cumsum(vdeg)])
    ell = np.zeros((n, N))
    use = slot >= 0
    ell[:, use] = -lam[:, slot[use]]
    odd = (deg[chk] & 1).astype(bool)
    P = ell.copy()
    R = np.zeros((n, E))
    x = np.zeros((n, N), dtype=np.uint8)
    its = np.zeros(n, dtype=np.int32)
    act = np.arange(n)
    with np.errstate(invalid="ignore"):
        for _ in range(int(code.max_iter)):
            if act.size == 0:
                break
            Pa, Ra = P[act], R[act]
            na = act.size
            m1 = np.full((na, M), np.inf)
            m2 = np.full((na, M), np.inf)
            i1 = np.zeros((na, M), dtype=np.int64)
            sg = np.zeros((na, M), dtype=bool)
            sgn = np.zeros((na, E), dtype=bool)
            for p in range(int(deg.max())):
                cs = np.flatnonzero(deg > p)
                e = row_ptr[cs] + p
                q = Pa[:, col[e]] - Ra[:, e]
                a = np.abs(q)
                s = q < 0
                sgn[:, e] = s
                c1, c2 = m1[:, cs], m2[:, cs]
                lt1 = a < c1
                lt2 = ~lt1 & (a < c2)
                m2[:, cs] = np.where(lt1, c1, np.where(lt2, a, c2))
                m1[:, cs] = np.where(lt1, a, c1)
                i1[:, cs] = np.where(lt1, p, i1[:, cs])
                sg[:, cs] ^= s
            mu = np.where(pos[None, :] == i1[:, chk], m2[:, chk], m1[:, chk])
            if _mutate == "no_exclude":
                mu = m1[:, chk]
            r = mu if _mutate == "alpha_late" else alpha * mu
            neg = sg[:, chk] ^ sgn
            if _mutate == "sign":
                neg = neg ^ odd[None, :]
            Rn = np.where(neg, -r, r)
            acc = ell[act].copy()
            for k in range(int(vdeg.max()) if E else 0):
                vs = np.flatnonzero(vdeg > k)
                acc[:, vs] = acc[:, vs] + Rn[:, by_var[vptr[vs] + k]]
            if _mutate == "alpha_late":
                acc = alpha * acc
            xa = (acc < 0).astype(np.uint8)
            P[act], R[act], x[act] = acc, Rn, xa
            its[act] += 1
            if code.early_stop:
                act = act[ldpc_syndrome(xa, code).any(axis=1)]
    return (x[0], its[0]) if single else (x, its)


def ldpc_counts(llr, sym, code, layers=None):
    """The definition of dsce_run_ldpc on exported arrays: llr [n][n_snr][S][ND][m]
    (export_llr) and sym [n][ND] (export) -> dict(bit_err, frame_err, iter_sum), int64
    [n_snr][S].  lam as in coded_counts; the decided information bits of the all-zero
    codeword and the iterations performed are counted.  With layers = (layer_ptr,
    layer_check) the definition of dsce_run_ldpc_layered: ldpc_decode_layered decodes."""
    llr = np.asarray(llr, dtype=np.float64)
    n, nk, S, nd, m = llr.shape
    t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(n, 1, 1, nd * m)
    flat = llr.reshape(n, nk, S, nd * m)
    lam = np.where(t, -flat, flat)
    lam = lam.reshape(n * nk * S, nd * m)
    x, it = ldpc_decode(lam, code) if layers is None else ldpc_decode_layered(lam, code, layers)
    bit = x[:, :code.n_info].astype(np.int64).sum(axis=1)
    return dict(bit_err=bit.reshape(n, nk, S).sum(axis=0), frame_err=(bit > 0).astype(np.int64).reshape(n, nk, S).sum(axis=0),
                iter_sum=it.astype(np.int64).reshape(n, nk, S).sum(axis=0))


# ---- the layered schedule (include/dsce.h, DSCE_HAS_LDPC_LAYERED) ----

def make_layers(code):
    """A layer partition of the checks of `code` for dsce_run_ldpc_layered /
    dsce_ldpc_layered by first fit in check order: check c goes to the lowest-numbered
    layer none of whose checks shares a variable with it, else it opens a new layer.
    Returns (layer_ptr int32 [n_layers + 1], layer_check int32 [n_checks]): the checks of
    layer l are layer_check[layer_ptr[l] : layer_ptr[l + 1]], ascending.  Deterministic."""
    row_ptr = np.asarray(code.row_ptr, dtype=np.int64)
    col = np.asarray(code.col, dtype=np.int64)
    used = [0] * int(code.n_vars)                           # per variable: bit l set = a check of layer l holds it
    layers = []
    for c in range(int(code.n_checks)):
        vs = col[row_ptr[c]:row_ptr[c + 1]].tolist()
        taken = 0
        for v in vs:
            taken |= used[v]
        l = (~taken & (taken + 1)).bit_length() - 1          # the lowest clear bit
        if l == len(layers):
            layers.append([])
        layers[l].append(c)
        for v in vs:
            used[v] |= 1 << l
    layer_ptr = np.concatenate([[0], np.cumsum([len(x) for x in layers])]).astype(np.int32)
    layer_check = np.array([c for x in layers for c in x], dtype=np.int32)
    return layer_ptr, layer_check


def serial_layers(code):
    """One check per layer, in check order: the serial schedule, valid for every code."""
    M = int(code.n_checks)
    return np.arange(M + 1, dtype=np.int32), np.arange(M, dtype=np.int32)


def check_layers(code, layers):
    """The host's checks of a layer partition (include/dsce.h), in its order and with its
    words: ValueError naming the offender.  Returns (layer_ptr, layer_check) as int64."""
    if layers is None or layers[0] is None or layers[1] is None:
        raise ValueError("null layers, layer_ptr or layer_check")
    lp = np.asarray(layers[0], dtype=np.int64).reshape(-1)
    lc = np.asarray(layers[1], dtype=np.int64).reshape(-1)
    M, L = int(code.n_checks), lp.size - 1
    if L < 1 or L > M:
        raise ValueError("n_layers outside 1 .. n_checks")
    if lc.size != M:
        raise ValueError("layer_check must have n_checks entries")
    if lp[0] != 0:
        raise ValueError("layer_ptr[0] is not 0")
    for l in range(L):
        if lp[l + 1] <= lp[l]:
            raise ValueError("layer_ptr gives layer %d no check" % l)
    if lp[L] != M:
        raise ValueError("layer_ptr[n_layers] is not n_checks")
    row_ptr = np.asarray(code.row_ptr, dtype=np.int64)
    col = np.asarray(code.col, dtype=np.int64)
    seen = np.zeros(M, dtype=bool)
    stamp = np.full(int(code.n_vars), -1, dtype=np.int64)   # the layer that last held the variable, and its check
    owner = np.zeros(int(code.n_vars), dtype=np.int64)
    for l in range(L):
        for c in lc[lp[l]:lp[l + 1]].tolist():
            if c < 0 or c >= M:
                raise ValueError("layer_check entry outside [0, n_checks)")
            if seen[c]:
                raise ValueError("check %d appears twice in layer_check" % c)
            seen[c] = True
            for v in col[row_ptr[c]:row_ptr[c + 1]].tolist():
                if stamp[v] == l:
                    raise ValueError("layer %d: checks %d and %d share variable %d" % (l, owner[v], c, v))
                stamp[v], owner[v] = l, c
    return lp, lc


def ldpc_decode_layered(lam, code, layers, _mutate=None):
    """Layered normalised min-sum decoding of lam [n_cw][n_slots] (or [n_slots]) under
    `code` with the layer partition `layers` = (layer_ptr, layer_check) (make_layers): (x
    uint8 [n_cw][n_vars], it int32 [n_cw]).  The twin of k_ldpc_layered, in fp64 and in
    the order of include/dsce.h: P = ell, R = 0; an iteration runs the layers in order,
    and for every check of a layer, over its edge positions p, q_p = P_v - R_p, the
    record (m1, i1, m2, sg, s_p) and R'_p exactly as in ldpc_decode, then P_v = q_p + R'_p
    and R_p = R'_p; after the last layer x = P < 0, and with early_stop a codeword stops
    once H x = 0.  The checks of a layer share no variable, so they are taken at once.
    _mutate is for the tests only: 'stale' (every check reads the P of the iteration's
    start: flooding) and 'no_store' (R' is never stored)."""
    lp, lc = check_layers(code, layers)
    lam = np.asarray(lam, dtype=np.float64)
    single = lam.ndim == 1
    lam = np.ascontiguousarray(lam.reshape(-1, lam.shape[-1]))
    n, N = lam.shape[0], code.n_vars
    row_ptr = np.asarray(code.row_ptr, dtype=np.int64)
    col = np.asarray(code.col, dtype=np.int64)
    slot = np.asarray(code.slot, dtype=np.int64)
    alpha = float(code.alpha)
    deg = np.diff(row_ptr)
    ell = np.zeros((n, N))
    use = slot >= 0
    ell[:, use] = -lam[:, slot[use]]
    # per layer: the edges of its checks as [checks][widest degree], the positions past a degree masked out
    plan = []
    for l in range(lp.size - 1):
        cs = lc[lp[l]:lp[l + 1]]
        pos = np.arange(int(deg[cs].max()))
        real = pos[None, :] < deg[cs][:, None]
        e = np.where(real, row_ptr[cs][:, None] + pos[None, :], 0)
        plan.append((e, col[e], real, pos[None, None, :], e[real], col[e[real]]))
    P = ell.copy()
    R = np.zeros((n, col.size))
    x = np.zeros((n, N), dtype=np.uint8)
    its = np.zeros(n, dtype=np.int32)
    act = np.arange(n)
    with np.errstate(invalid="ignore"):
        for _ in range(int(code.max_iter)):
            if act.size == 0:
                break
            Pa, Ra = P[act], R[act]
            P0 = Pa.copy() if _mutate == "stale" else None
            for e, v, real, pos, er, vr in plan:
                q = (Pa if P0 is None else P0)[:, v] - Ra[:, e]
                a = np.where(real, np.abs(q), np.inf)
                s = (q < 0) & real
                i1 = a.argmin(axis=2)[:, :, None]              # the first of equal minima: the lowest position
                m1 = np.take_along_axis(a, i1, axis=2)
                np.put_along_axis(a, i1, np.inf, axis=2)
                m2 = a.min(axis=2)[:, :, None]
                sg = np.logical_xor.reduce(s, axis=2)[:, :, None]
                r = alpha * np.where(pos == i1, m2, m1)
                Rn = np.where(sg ^ s, -r, r)
                if P0 is None:
                    Pa[:, vr] = (q + Rn)[:, real]
                else:
                    Pa[:, vr] = Pa[:, vr] + (Rn[:, real] - Ra[:, er])
                if _mutate != "no_store":
                    Ra[:, er] = Rn[:, real]
            xa = (Pa < 0).astype(np.uint8)
            P[act], R[act], x[act] = Pa, Ra, xa
            its[act] += 1
            if code.early_stop:
                act = act[ldpc_syndrome(xa, code).any(axis=1)]
    return (x[0], its[0]) if single else (x, its)


# ---- the flooding decoder in fixed point (include/dsce.h, DSCE_HAS_LDPC_FIXED) ----

LdpcFixed = collections.namedtuple("LdpcFixed", "scale q_ch q_msg q_app alpha_num alpha_shift beta")
LdpcFixed.__doc__ = """The word lengths and the rule of dsce_run_ldpc_fixed / dsce_ldpc_fixed (dsce_ldpc_fixed_desc of
include/dsce.h): scale quantiser steps per LLR unit; q_ch, q_msg, q_app bits of the channel,
message and a-posteriori words (symmetric ranges +-(2^(q-1) - 1)); the normalisation
alpha_num / 2^alpha_shift, rounded half up; the offset beta."""


def make_fixed(q_ch=6, q_msg=6, q_app=8, scale=2.0, alpha_num=1, alpha_shift=0, beta=1):
    """An LdpcFixed, checked (check_fixed).  The defaults: 6 / 6 / 8 bit, two steps per LLR
    unit (a channel clip of 15.5), no normalisation, offset 1."""
    fx = LdpcFixed(float(scale), int(q_ch), int(q_msg), int(q_app), int(alpha_num), int(alpha_shift), int(beta))
    check_fixed(fx)
    return fx


def check_fixed(fx):
    """The host's checks of a dsce_ldpc_fixed_desc, in its order and with its words: ValueError
    naming the offender.  Returns (C, X, A)."""
    if fx is None:
        raise ValueError("null fx")
    if not (np.isfinite(fx.scale) and fx.scale > 0.0):
        raise ValueError("scale must be finite and > 0")
    if not 2 <= fx.q_ch <= 16:
        raise ValueError("q_ch outside 2 .. 16")
    if not 2 <= fx.q_msg <= 16:
        raise ValueError("q_msg outside 2 .. 16")
    if not max(fx.q_ch, fx.q_msg) <= fx.q_app <= 16:
        raise ValueError("q_app outside max(q_ch, q_msg) .. 16")
    if not 0 <= fx.alpha_shift <= 8:
        raise ValueError("alpha_shift outside 0 .. 8")
    if not 1 <= fx.alpha_num <= (1 << fx.alpha_shift):
        raise ValueError("alpha_num outside 1 .. 1 << alpha_shift")
    if not 0 <= fx.beta <= 32767:
        raise ValueError("beta outside 0 .. 32767")
    return tuple((1 << (q - 1)) - 1 for q in (fx.q_ch, fx.q_msg, fx.q_app))


def check_codeword(code, codeword):
    """The host's checks of the codeword of dsce_run_ldpc_fixed: ValueError naming the first
    entry that is not 0 or 1, or the first unsatisfied check.  Returns it as uint8 [n_vars]."""
    c = np.ascontiguousarray(np.asarray(codeword).reshape(-1), dtype=np.uint8)
    if c.size != int(code.n_vars):
        raise ValueError("codeword must have n_vars entries")
    if (c > 1).any():
        raise ValueError("codeword entry %d is not 0 or 1" % int(np.flatnonzero(c > 1)[0]))
    syn = ldpc_syndrome(c, code)
    if syn.any():
        raise ValueError("codeword does not satisfy check %d" % int(np.flatnonzero(syn)[0]))
    return c


def ldpc_fixed_lds_bytes(n_vars, n_checks):
    """Dynamic LDS bytes of k_ldpc_fixed per workgroup (DSCE_LDPC_FIXED_LDS_BYTES)."""
    return 4 * int(n_vars) + 10 * int(n_checks) + 8


def ldpc_quantise(lam, fx):
    """Step 1 of the fixed-point decoder on lam (any shape): int32 ell = Q(-lam): t = (-lam) *
    scale, magnitude min(floor(|t| + 0.5), C), the sign of t; NaN gives 0, +-inf saturates."""
    C = check_fixed(fx)[0]
    with np.errstate(invalid="ignore", over="ignore"):
        t = (-np.asarray(lam, dtype=np.float64)) * np.float64(fx.scale)
        a = np.abs(t)
        sat = a >= C                                          # False for NaN
        mag = np.where(sat, float(C), np.floor(np.where(sat | np.isnan(a), 0.0, a) + 0.5))
    mag = mag.astype(np.int32)
    return np.where(t < 0, -mag, mag).astype(np.int32)


def ldpc_decode_fixed(lam, code, fx, _mutate=None, _ell=None):
    """Fixed-point min-sum decoding of lam [n_cw][n_slots] (or [n_slots]; positive = the bit
    is 1) under `code` and the LdpcFixed `fx`: (x uint8 [n_cw][n_vars], it int32 [n_cw], P
    int16 [n_cw][n_vars]), the decided bits and the a-posteriori sums of the last iteration
    performed and the number of iterations.  The twin of k_ldpc_fixed, in the integers of
    include/dsce.h: ell = ldpc_quantise (0 for slot -1), P = ell, R = 0; per check q_p =
    clamp(P_v - R_p, +-X), the record of ldpc_decode on |q_p| and q_p < 0, r = max(((mu *
    alpha_num + half) >> alpha_shift) - beta, 0), R'_p = +-r; per variable P' = clamp(ell +
    sum R', +-A); x = P' < 0; with early_stop a codeword stops once H x = 0.  code.alpha is
    not read.  _ell (int [n_cw][n_vars]) replaces the quantiser's output (ldpc_counts_fixed).
    _mutate is for the tests only: 'trunc' (no rounding term), 'late_clamp' (q_p not
    clamped), 'beta_first' (the offset before the normalisation)."""
    C, X, A = check_fixed(fx)
    an, sh, beta = int(fx.alpha_num), int(fx.alpha_shift), int(fx.beta)
    half = 0 if _mutate == "trunc" else (1 << sh) >> 1
    N, M = code.n_vars, code.n_checks
    row_ptr = np.asarray(code.row_ptr, dtype=np.int64)
    col = np.asarray(code.col, dtype=np.int64)
    slot = np.asarray(code.slot, dtype=np.int64)
    if _ell is None:
        lam = np.asarray(lam, dtype=np.float64)
        single = lam.ndim == 1
        lam = lam.reshape(-1, lam.shape[-1])
        ell = np.zeros((lam.shape[0], N), dtype=np.int32)
        use = slot >= 0
        ell[:, use] = ldpc_quantise(lam[:, slot[use]], fx)
    else:
        ell = np.asarray(_ell, dtype=np.int32)
        single = ell.ndim == 1
        ell = ell.reshape(-1, N)
    n = ell.shape[0]
    deg = np.diff(row_ptr)
    E = col.size
    chk = np.repeat(np.arange(M), deg)
    pos = np.arange(E) - row_ptr[chk]
    by_var = np.argsort(col, kind="stable")                 # the edges grouped by variable
    vptr = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=N))])
    big = np.int32(0x7FFFFFFF)
    P = ell.copy()
    R = np.zeros((n, E), dtype=np.int32)
    x = np.zeros((n, N), dtype=np.uint8)
    its = np.zeros(n, dtype=np.int32)
    act = np.arange(n)
    for _ in range(int(code.max_iter)):
        if act.size == 0:
            break
        Pa, Ra = P[act], R[act]
        na = act.size
        m1 = np.full((na, M), big, dtype=np.int32)
        m2 = np.full((na, M), big, dtype=np.int32)
        i1 = np.zeros((na, M), dtype=np.int64)
        sg = np.zeros((na, M), dtype=bool)
        sgn = np.zeros((na, E), dtype=bool)
        for p in range(int(deg.max())):
            cs = np.flatnonzero(deg > p)
            e = row_ptr[cs] + p
            q = Pa[:, col[e]] - Ra[:, e]
            if _mutate != "late_clamp":
                q = np.clip(q, -X, X)
            a = np.abs(q)
            s = q < 0
            sgn[:, e] = s
            c1, c2 = m1[:, cs], m2[:, cs]
            lt1 = a < c1
            lt2 = ~lt1 & (a < c2)
            m2[:, cs] = np.where(lt1, c1, np.where(lt2, a, c2))
            m1[:, cs] = np.where(lt1, a, c1)
            i1[:, cs] = np.where(lt1, p, i1[:, cs])
            sg[:, cs] ^= s
        mu = np.where(pos[None, :] == i1[:, chk], m2[:, chk], m1[:, chk]).astype(np.int64)
        if _mutate == "beta_first":
            r = (np.maximum(mu - beta, 0) * an + half) >> sh
        else:
            r = np.maximum(((mu * an + half) >> sh) - beta, 0)
        r = r.astype(np.int32)
        Rn = np.where(sg[:, chk] ^ sgn, -r, r)
        run = np.concatenate([np.zeros((na, 1), dtype=np.int64), np.cumsum(Rn[:, by_var], axis=1, dtype=np.int64)], axis=1)
        acc = np.clip(ell[act] + (run[:, vptr[1:]] - run[:, vptr[:-1]]), -A, A).astype(np.int32)
        xa = (acc < 0).astype(np.uint8)
        P[act], R[act], x[act] = acc, Rn, xa
        its[act] += 1
        if code.early_stop:
            act = act[ldpc_syndrome(xa, code).any(axis=1)]
    P = P.astype(np.int16)
    return (x[0], its[0], P[0]) if single else (x, its, P)


def ldpc_counts_fixed(llr, sym, code, fx, codeword=None):
    """The definition of dsce_run_ldpc_fixed on exported arrays: llr [n][n_snr][S][ND][m]
    (export_llr) and sym [n][ND] (export) -> dict(bit_err, frame_err, iter_sum), int64
    [n_snr][S].  lam as in coded_counts, quantised (ldpc_quantise), negated where the
    codeword (uint8 [n_vars], checked; None = all zero) has a 1; ldpc_decode_fixed decodes,
    and the decided information bits that differ from the codeword are counted."""
    llr = np.asarray(llr, dtype=np.float64)
    n, nk, S, nd, m = llr.shape
    t = ((np.asarray(sym)[..., None] >> np.arange(m)) & 1).astype(bool).reshape(n, 1, 1, nd * m)
    flat = llr.reshape(n, nk, S, nd * m)
    lam = np.where(t, -flat, flat).reshape(n * nk * S, nd * m)
    c = np.zeros(int(code.n_vars), dtype=np.uint8) if codeword is None else check_codeword(code, codeword)
    slot = np.asarray(code.slot, dtype=np.int64)
    ell = np.zeros((lam.shape[0], int(code.n_vars)), dtype=np.int32)
    use = slot >= 0
    ell[:, use] = ldpc_quantise(lam[:, slot[use]], fx)
    ell = np.where(c[None, :].astype(bool), -ell, ell)
    x, it, P = ldpc_decode_fixed(None, code, fx, _ell=ell)
    bit = (x ^ c[None, :])[:, :code.n_info].astype(np.int64).sum(axis=1)
    return dict(bit_err=bit.reshape(n, nk, S).sum(axis=0), frame_err=(bit > 0).astype(np.int64).reshape(n, nk, S).sum(axis=0),
                iter_sum=it.astype(np.int64).reshape(n, nk, S).sum(axis=0))
