"""Second moments of per-realisation samples against an analytic matrix, scored in
standard errors (tests/test_moments_host.py, tests/test_gpu_moments.py).  Plain
NumPy: no engine and no oracle is imported here.

For samples a [n][A] and b [n][B] the product p_ij = a_i conj(b_j) has the mean
m_ij = (1/n) sum p_ij, and, the realisations being independent, m_ij has the
standard error

    se_ij = sqrt((mean |p_ij|^2 - |m_ij|^2) / n),

with the variance estimated from the samples themselves: no Gaussian assumption
(one path per tap gives a channel of constant modulus per tap, far from Gaussian,
and the statistic must hold there too).  Both sums are matrix products, a^T
conj(b) and (|a|^2)^T |b|^2, so no n x A x B tensor is ever formed and the
samples may arrive in chunks.

The score of an entry is z = |m - analytic| / se.  BAR = 6 is derived, not
measured: by the central limit theorem m is normal around its expectation; a
real entry (a diagonal one: a power) lies beyond 6 se with probability
erfc(6 / sqrt 2) = 2.0e-9, a circular complex one, whose se^2 is the sum of both
components' variances, with probability exp(-36) = 2.3e-16, and no case of the
two test files asserts more than 10^5 entries: a false alarm per case has
probability below 2e-4 and, the seeds being fixed, happens never or always.  An
entry over the bar is therefore a finding to be explained, never settled by
another seed or a wider bar."""
import numpy as np

BAR = 6.0


class Moments:
    """Accumulates sum a_i conj(b_j) and sum |a_i|^2 |b_j|^2 over chunks."""

    def __init__(self, A, B):
        self.s1 = np.zeros((A, B), dtype=np.complex128)
        self.s2 = np.zeros((A, B), dtype=np.float64)
        self.n = 0

    def add(self, a, b):
        a = np.asarray(a, dtype=np.complex128)
        b = np.asarray(b, dtype=np.complex128)
        assert a.ndim == b.ndim == 2 and a.shape[0] == b.shape[0], (a.shape, b.shape)
        assert (a.shape[1], b.shape[1]) == self.s1.shape, (a.shape, b.shape, self.s1.shape)
        self.s1 += a.T @ b.conj()
        self.s2 += (a.real ** 2 + a.imag ** 2).T @ (b.real ** 2 + b.imag ** 2)
        self.n += a.shape[0]
        return self

    def mean(self):
        return self.s1 / self.n

    def se(self):
        m = self.mean()
        var = self.s2 / self.n - (m.real ** 2 + m.imag ** 2)
        return np.sqrt(np.maximum(var, 0.0) / self.n)

    def z(self, analytic=0.0):
        return score(self.mean(), self.se(), analytic)


def score(mean, se, analytic=0.0):
    """|mean - analytic| / se per entry; an entry without spread scores 0 where it is met
    exactly and inf where it is not."""
    d = np.abs(mean - analytic)
    with np.errstate(divide="ignore", invalid="ignore"):
        z = d / se
    return np.where(se > 0, z, np.where(d == 0, 0.0, np.inf))


def worst(z, mask=None):
    """(max z, its index) over the entries of mask (all by default)."""
    z = np.asarray(z, dtype=np.float64)
    zz = z if mask is None else np.where(mask, z, -1.0)
    at = np.unravel_index(int(np.argmax(zz)), zz.shape)
    return float(zz[at]), tuple(int(i) for i in at)


class Families:
    """The four families of one scheme over n_snr SNR points, fed by chunks of
    h [n][LK], hp_ls [n][n_snr][NP] and h_est [n][n_snr][LK]:

      a   E{h_i conj(h_j)} over the pilot positions                  -> R_hP
      b   E{h_c conj(h_p)}, every position c, every pilot p          -> rows (c, c) of R_Dij
      c   E{hp_ls hp_ls^H} per SNR point: the diagonal               -> diag R_est[k]
          (off: its off-diagonal, exact for OFDM only                -> R_est[k])
      d   E{(h_est_c - h_c) conj(hp_ls_j)} per SNR point             -> 0
    """

    def __init__(self, lk, pilot_pos, n_snr):
        self.pilot_pos = np.asarray(pilot_pos)
        npil = self.pilot_pos.size
        self.b = Moments(lk, npil)                                  # a is its rows at the pilots
        self.c = [Moments(npil, npil) for _ in range(n_snr)]
        self.d = [Moments(lk, npil) for _ in range(n_snr)]

    def add(self, h, hp_ls, h_est):
        self.b.add(h, h[:, self.pilot_pos])
        for k in range(len(self.c)):
            self.c[k].add(hp_ls[:, k], hp_ls[:, k])
            self.d[k].add(h_est[:, k] - h, hp_ls[:, k])
        return self

    @property
    def n(self):
        return self.b.n

    def scores(self, R_hP, R_Dij_cc, R_est):
        """max z per family against R_hP [NP][NP], R_Dij_cc [LK][NP] (the rows (c, c) of
        R_Dij) and R_est [n_snr][NP][NP]: dict a, b, c, off, d -> (max z, index)."""
        npil = self.pilot_pos.size
        eye = np.eye(npil, dtype=bool)
        pp = self.pilot_pos
        zb = self.b.z(R_Dij_cc)
        zc = np.stack([m.z(R_est[k]) for k, m in enumerate(self.c)])
        zd = np.stack([m.z(0.0) for m in self.d])
        return dict(a=worst(score(self.b.mean()[pp], self.b.se()[pp], R_hP)),
                    b=worst(zb), c=worst(zc, eye[None]), off=worst(zc, ~eye[None]) if npil > 1 else (0.0, (0, 0, 0)),
                    d=worst(zd))


def diag_rows(W, lk, npil):
    """The rows (c, c) of a vector in the reference's layout r + LK c + LK^2 p (a column of
    W or W0; R_Dij [LK^2][NP] flattened column-major) as an [LK][NP] array."""
    W = np.asarray(W).reshape(-1)
    assert W.size == lk * lk * npil, (W.size, lk, npil)
    return W.reshape(npil, lk * lk)[:, ::lk + 1].T.copy()
