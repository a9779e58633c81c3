// kernels_llr.hip — soft outputs: SignalConstellation.LLR_AWGN
// (SignalConstellation.m:103-122) as defined in include/dsce.h, for single points
// (k_llr_probe; dsce_llr_awgn) and in bulk for every stage of the MMSE branch
// or of the perfect-CSI branch (LlrK::perfect; DSCE_LLR_PERFECT)
// (k_llr; dsce_export_llr), and the BICM information loss summed from those LLRs
// on the device (k_llr_info + k_llr_info_sum; dsce_run_soft).  One device
// function, llr_demap, serves all of them.  k_llr_calib (dsce_run_calib) sums the
// demapper error against the transmitted symbol over pn_eff instead; it shares
// the demapper input (llr_input) with the two bulk kernels.
//
//   LLR_b(x, pn) = log sum_{bit_b = 1} exp(-e_i) - log sum_{bit_b = 0} exp(-e_i),   e_i = |x - s_i|^2 / pn
//
// Per-axis form (LlrTab::per_axis, every Gray map of the reference): a bit that
// depends on one axis of the grid only sees the other axis' factor in both sums,
// so it cancels and the LLR is a PAM LLR over that axis' <= 16 levels:
// e_i = (c - lv_i)^2 / pn, one shift by min e_i, t_i = exp(-(e_i - min)) once per
// level and shared by the axis' bits, masked sums per bit: <= 32 exponentials per
// symbol instead of 256 per bit.  A set whose shared-shift sum falls below
// LLR_TINY (every member more than ~667 above the minimum) is summed again with
// its own minimum as the shift, so the result stays finite and accurate for every
// finite x and pn > 0.  The full-table form does the same over all M symbols.
// Max-log takes the masked minima of the squared distances and divides their
// difference by pn once.  NaN in gives NaN out.
// Plain IEEE division and the library exp / log in fp64.
#include "dsce_kernels.h"

#include <math.h>

namespace dsce {

static constexpr double LLR_TINY = 1e-290;   // exp(-667.7); normal doubles reach 2.2e-308

// log sum_{i in set} exp(-(e_i - emin)) of one axis: log(s) with the shared-shift
// sum s, or from the set's own minimum mset when s is too small to hold it
__device__ __forceinline__ double axis_set_log(double s, double mset, double emin, const double (&e)[16], unsigned set) {
    if (s < LLR_TINY) {
        double r = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((set >> i) & 1) r += exp(-(e[i] - mset));
        return log(r) - (mset - emin);
    }
    return log(s);
}

// the bits of axis ax (component c of the observation); store(b, llr)
template <class Store>
__device__ __forceinline__ void llr_axis(const LlrTab& t, int ax, double c, double pn, bool maxlog, Store store) {
    const int n = ax ? t.nQ : t.nI;
    const double* lv = ax ? t.lvQ : t.lvI;
    double e[16], tt[16];
    double emin = INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const double d = c - lv[i];
        // max-log divides the difference of the minima once; a level past n: weight 0 in every sum and minimum
        e[i] = i < n ? (maxlog ? d * d : d * d / pn) : INFINITY;
        emin = fmin(emin, e[i]);
    }
    if (!maxlog) {
#pragma unroll
        for (int i = 0; i < 16; ++i) tt[i] = exp(-(e[i] - emin));
    }
    const unsigned all = (1u << n) - 1u;
    for (int b = 0; b < t.m; ++b) {
        if (t.axis[b] != ax) continue;
        const unsigned one = t.mask[b], zero = all & ~one;
        double m1 = INFINITY, m0 = INFINITY, s1 = 0.0, s0 = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const bool in1 = (one >> i) & 1, in0 = (zero >> i) & 1;
            m1 = in1 ? fmin(m1, e[i]) : m1;
            m0 = in0 ? fmin(m0, e[i]) : m0;
            if (!maxlog) {
                s1 += in1 ? tt[i] : 0.0;
                s0 += in0 ? tt[i] : 0.0;
            }
        }
        // NaN input: fmin skips it, so the minima stay Inf and Inf - Inf = NaN
        store(b, maxlog ? (m0 - m1) / pn : axis_set_log(s1, m1, emin, e, one) - axis_set_log(s0, m0, emin, e, zero));
    }
}

__device__ __forceinline__ double table_d2(const LlrTab& t, int i, double2 x) {
    const double2 s = t.symbols[i];
    const double dx = x.x - s.x, dy = x.y - s.y;
    return dx * dx + dy * dy;
}
__device__ __forceinline__ double table_e(const LlrTab& t, int i, double2 x, double pn) { return table_d2(t, i, x) / pn; }

// the full-table form: every bit over all M symbols (a labelling that is not axis-pure)
template <class Store>
__device__ __forceinline__ void llr_table(const LlrTab& t, double2 x, double pn, bool maxlog, Store store) {
    double m1[8], m0[8], s1[8], s0[8];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        m1[b] = m0[b] = INFINITY;
        s1[b] = s0[b] = 0.0;
    }
    double emin = INFINITY;
    for (int i = 0; i < t.M; ++i) {
        const double e = maxlog ? table_d2(t, i, x) : table_e(t, i, x, pn);   // max-log: one division at the end
        emin = fmin(emin, e);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (i >> b) & 1;
            m1[b] = bit ? fmin(m1[b], e) : m1[b];
            m0[b] = bit ? m0[b] : fmin(m0[b], e);
        }
    }
    if (!maxlog)
        for (int i = 0; i < t.M; ++i) {
            const double w = exp(-(table_e(t, i, x, pn) - emin));
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const bool bit = (i >> b) & 1;
                s1[b] += bit ? w : 0.0;
                s0[b] += bit ? 0.0 : w;
            }
        }
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        if (b >= t.m) break;
        if (maxlog) {
            store(b, (m0[b] - m1[b]) / pn);
            continue;
        }
        double l[2];
#pragma unroll
        for (int v = 0; v < 2; ++v) {
            const double s = v ? s1[b] : s0[b], ms = v ? m1[b] : m0[b];
            if (s < LLR_TINY) {                        // the set again, shifted by its own minimum
                double r = 0.0;
                for (int i = 0; i < t.M; ++i)
                    if (((i >> b) & 1) == v) r += exp(-(table_e(t, i, x, pn) - ms));
                l[v] = log(r) - (ms - emin);
            } else {
                l[v] = log(s);
            }
        }
        store(b, l[1] - l[0]);
    }
}

// the m LLRs of observation x with noise power pn: store(b, LLR_b), b = 0 .. m - 1
template <class Store>
__device__ __forceinline__ void llr_demap(const LlrTab& t, double2 x, double pn, bool maxlog, Store store) {
    if (t.per_axis) {
        // 0 for finite x; a NaN in either component reaches the bits of both axes, as in the full table
        const double nanp = 0.0 * (x.x + x.y);
        if (t.nbit[0]) llr_axis(t, 0, x.x + nanp, pn, maxlog, store);
        if (t.nbit[1]) llr_axis(t, 1, x.y + nanp, pn, maxlog, store);
    } else {
        llr_table(t, x, pn, maxlog, store);
    }
}

__global__ void __launch_bounds__(256) k_llr_probe(LlrTab t, const double2* __restrict__ x,
                                                   const double* __restrict__ pn, long long n_pn, long long n,
                                                   int maxlog, double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        double* o = out + i * t.m;
        llr_demap(t, x[i], pn[n_pn == 1 ? 0 : i], maxlog != 0, [&](int b, double v) { o[b] = v; });
    }
}

void launch_llr_probe(hipStream_t s, const LlrTab& t, const double2* x, const double* pn, long long n_pn, long long n,
                      bool maxlog, double* out) {
    if (n <= 0) return;
    const int blocks = (int)std::min<long long>((n + 255) / 256, 1 << 16);
    hipLaunchKernelGGL(k_llr_probe, dim3(blocks), dim3(256), 0, s, t, x, pn, n_pn, n, maxlog ? 1 : 0, out);
}

// The demapper input of data symbol j for the lane's unit, as include/dsce.h
// defines it: x_est and the AWGN pn_eff from row(s) base + l of ysrc [..][U] at
// `unit` and row(s) hbase + l of hsrc [..][hU] at `hunit` (y_ic and h_est of the
// stage; or y_perf of the stage, y for stage 0 and the pseudo-stage, with the
// batch's perfect-CSI diag(D): LlrSrc below).  One statement sequence for k_llr,
// k_llr_info and k_llr_calib and for both branches, so all form the same bits.
__device__ __forceinline__ void llr_input(const LlrK& a, const double2* __restrict__ ysrc, size_t base, size_t U,
                                          size_t unit, const double2* __restrict__ hsrc, size_t hbase, size_t hU,
                                          size_t hunit, int j, double pnk, double2& x, double& pe) {
    if (a.despread) {                                      // x = P^H (y ./ h), row NP + j of P^H
        double2 acc = make_double2(0.0, 0.0);
        double pacc = 0.0;
        const int j0 = a.ph_ptr[a.NP + j], j1 = a.ph_ptr[a.NP + j + 1];
        for (int jj = j0; jj < j1; ++jj) {
            const int l = a.ph_col[jj];
            const double2 pv = a.ph_val[jj];
            const double2 y = ysrc[(base + l) * U + unit], h = hsrc[(hbase + l) * hU + hunit];
            c_fma(acc, pv, c_div(y, h));
            pacc += (pv.x * pv.x + pv.y * pv.y) * (pnk * a.qn[l]) / (h.x * h.x + h.y * h.y);
        }
        x = make_double2(acc.x / a.data_div, acc.y / a.data_div);
        pe = pacc / (a.data_div * a.data_div);
    } else {
        const int l = a.data_pos[j];
        const double2 y = ysrc[(base + l) * U + unit], h = hsrc[(hbase + l) * hU + hunit];
        const double2 q = c_div(y, h);
        x = make_double2(q.x / a.data_div, q.y / a.data_div);
        pe = pnk * a.qn[l] / ((h.x * h.x + h.y * h.y) * (a.data_div * a.data_div));
    }
    if (a.real_detect) x.y = 0.0;
}

// Where stage `stage` of 0 .. S reads its observation and its channel (block-
// uniform).  MMSE branch: y_ic and h_est of the stage, [S][LK][U].  Perfect CSI
// (the pseudo-stage S, or every stage with LlrK::perfect): y_perf of the stage,
// y = stage 0 of y_ic for stage 0 and the pseudo-stage, and diag(D) h[l][rep].
struct LlrSrc {
    const double2* y;
    const double2* h;
    size_t base, hbase, hU;
    bool perf;
};
__device__ __forceinline__ LlrSrc llr_src(const LlrK& a, int stage) {
    LlrSrc r;
    const bool pseudo = stage == a.S;
    r.perf = pseudo || a.perfect != 0;
    r.y = (r.perf && !pseudo && stage > 0) ? a.yperf : a.yic;
    r.base = pseudo ? 0 : (size_t)stage * a.LK;
    r.h = r.perf ? a.h : a.hest;
    r.hbase = r.perf ? 0 : r.base;
    r.hU = r.perf ? (size_t)a.R : (size_t)a.U;
    return r;
}

// k_llr — the sibling of k_export_stages for the soft outputs.  One block = 64
// consecutive units (one SNR point) x one tile of LT data symbols of one stage.
// Phase 1, lane = unit, wave w the tile's symbols w, w + 4, ..: y_ic and h_est of
// the symbol's rows are read element-major (64 x 16 B contiguous per row), x_est
// and pn_eff formed as include/dsce.h defines them, the symbol demapped, and the
// results go to LDS as tile[unit][element] with odd row strides (LT + 1 slots;
// LT m + 1 doubles).  Phase 2, lane = output element: LT consecutive symbols (LT m
// consecutive LLRs) of a realisation per store group.  LT = 16 for m <= 4, 8
// above, which keeps the block within 64 KiB of LDS.
template <bool F32, int LT>
__global__ void __launch_bounds__(256) k_llr(LlrK a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int XS = LT + 1;
    double2* xt = (double2*)smem;                          // [64][XS]
    double* pt = (double*)(smem + 64 * XS * 16);           // [64][XS]
    double* lt = (double*)(smem + 64 * XS * 24);           // [64][LT m + 1]
    const int m = a.tab.m, LS = LT * m + 1;
    const int ntile = (a.ND + LT - 1) / LT;
    const int stage = blockIdx.y / ntile, e0 = (blockIdx.y % ntile) * LT;
    const int first = blockIdx.x * 64;                     // first unit of the block (one SNR point: R % 64 == 0)
    const int snr = a.snr0 + first / a.R;
    const int rl0 = first % a.R;
    const int nv = min(64, a.rvalid - rl0);                // realisations of the group that are written
    if (nv <= 0) return;                                   // a wave of tail padding (block-uniform)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t U = (size_t)a.U, unit = (size_t)first + lane;
    const LlrSrc sr = llr_src(a, stage);
    const size_t hunit = sr.perf ? (size_t)(rl0 + lane) : unit;
    const double pnk = a.pn[snr];
    const bool want_llr = a.out[2] != nullptr;
    for (int e = w; e < LT; e += 4) {
        const int j = e0 + e;
        if (j >= a.ND) break;                              // wave-uniform
        double2 x;
        double pe;
        llr_input(a, sr.y, sr.base, U, unit, sr.h, sr.hbase, sr.hU, hunit, j, pnk, x, pe);
        if (a.scale) pe = a.scale[((size_t)snr * a.S + stage) * a.ND + j] * pe;   // wave-uniform load
        xt[lane * XS + e] = x;
        pt[lane * XS + e] = pe;
        if (want_llr) {
            double* o = lt + lane * LS + e * m;
            llr_demap(a.tab, x, pe, a.maxlog != 0, [&](int b, double v) { o[b] = v; });
        }
    }
    __syncthreads();

    const size_t ND = (size_t)a.ND;
    // lane = symbol: LT consecutive symbols of one realisation per lane group
    {
        const int e = threadIdx.x & (LT - 1);
        if (e0 + e < a.ND)
            for (int u = threadIdx.x / LT; u < nv; u += 256 / LT) {
                const long long row = a.row0 + rl0 + u;
                const size_t idx = ((size_t)(row * a.nsnr + snr) * a.S + stage) * ND + (size_t)(e0 + e);
                if (a.out[0]) {
                    const double2 v = xt[u * XS + e];
                    if (F32) ((float2*)a.out[0])[idx] = make_float2((float)v.x, (float)v.y);
                    else ((double2*)a.out[0])[idx] = v;
                }
                if (a.out[1]) {
                    const double v = pt[u * XS + e];
                    if (F32) ((float*)a.out[1])[idx] = (float)v;
                    else ((double*)a.out[1])[idx] = v;
                }
            }
    }
    // lane = LLR: the tile's min(LT, ND - e0) m consecutive LLRs of one realisation
    if (want_llr) {
        const int rowlen = min(LT, a.ND - e0) * m;
        for (int k = threadIdx.x; k < nv * rowlen; k += 256) {
            const int u = k / rowlen, i = k - u * rowlen;
            const long long row = a.row0 + rl0 + u;
            const size_t idx = (((size_t)(row * a.nsnr + snr) * a.S + stage) * ND + (size_t)e0) * m + (size_t)i;
            const double v = lt[u * LS + i];
            if (F32) ((float*)a.out[2])[idx] = (float)v;
            else ((double*)a.out[2])[idx] = v;
        }
    }
}

template <int LT>
static void launch_llr_lt(hipStream_t s, const LlrK& a, bool f32) {
    const dim3 grid(a.U / 64, a.S * ((a.ND + LT - 1) / LT));
    const size_t lds = (size_t)64 * (LT + 1) * 24 + (size_t)64 * (LT * a.tab.m + 1) * 8;
    if (f32) hipLaunchKernelGGL((k_llr<true, LT>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((k_llr<false, LT>), grid, dim3(256), lds, s, a);
}

void launch_llr(hipStream_t s, const LlrK& a, bool f32) {
    if (!a.out[0] && !a.out[1] && !a.out[2]) return;
    if (a.tab.m <= 4) launch_llr_lt<16>(s, a, f32);
    else launch_llr_lt<8>(s, a, f32);
}

// loss_b ln 2 = log(1 + exp(-z)), z = (2 t_b - 1) LLR_b, in the stable form of
// include/dsce.h: finite for every finite LLR, NaN for NaN (fmax drops it, exp keeps it)
__device__ __forceinline__ double info_loss_nats(double llr, bool bit) {
    const double z = bit ? llr : -llr;
    return fmax(-z, 0.0) + log1p(exp(-fabs(z)));
}

// k_llr_info — k_llr with a sum in place of the stores.  Phase 1 is k_llr's
// (llr_input; lane = unit, wave w the tile's symbols w, w + 4, ..),
// with the channel of pseudo-stage S read from h[l][rep]; the store callback
// adds the bit's loss, in nats, to the lane's two fp64 sums (all symbols,
// considered symbols) with the transmitted index sidx[j][rep], contiguous across
// the wave.  No transpose, so no LDS tile: LLR_INFO_LT symbols per block.  The
// block's lanes are summed by a fixed butterfly per wave and in wave order
// through LDS, divided by ln 2 once, and go to the block's own slot of `part`.
__global__ void __launch_bounds__(256) k_llr_info(LlrInfoK q) {
    __shared__ double red[4][2];
    constexpr int LT = LLR_INFO_LT;
    const LlrK& a = q.k;
    const int ntile = (a.ND + LT - 1) / LT;
    const int st = blockIdx.y / ntile, tile = blockIdx.y % ntile, e0 = tile * LT;
    const int stage = q.st_lo + st;
    const bool pseudo = stage == a.S;                      // the perfect-CSI one-tap receiver
    const int first = blockIdx.x * 64;                     // first unit of the block (one SNR point: R % 64 == 0)
    const int sc = first / a.R, snr = a.snr0 + sc;
    const int rl0 = first % a.R;
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int rep = rl0 + lane;
    const bool counts = rep < a.rvalid;                    // a padding realisation adds nothing
    const size_t U = (size_t)a.U, unit = (size_t)first + lane;
    const LlrSrc sr = llr_src(a, stage);
    const size_t hunit = sr.perf ? (size_t)rep : unit;
    const double pnk = a.pn[snr];
    // the scale row of (snr, stage): a.scale (g_est, or g_perf of the perfect-CSI branch), g_perf0 for the pseudo-stage
    const double* scale = pseudo ? (q.scale_perf ? q.scale_perf + (size_t)snr * a.ND : nullptr)
                               : (a.scale ? a.scale + ((size_t)snr * a.S + stage) * a.ND : nullptr);
    double sum_all = 0.0, sum_con = 0.0;
    if (rl0 < a.rvalid)                                    // else a wave of tail padding (block-uniform)
        for (int e = w; e < LT; e += 4) {
            const int j = e0 + e;
            if (j >= a.ND) break;                          // wave-uniform
            double2 x;
            double pe;
            llr_input(a, sr.y, sr.base, U, unit, sr.h, sr.hbase, sr.hU, hunit, j, pnk, x, pe);
            if (scale) pe = scale[j] * pe;                 // wave-uniform load
            const unsigned t = q.sidx[(size_t)j * a.R + rep];
            double sym = 0.0;
            llr_demap(a.tab, x, pe, a.maxlog != 0, [&](int b, double v) { sym += info_loss_nats(v, (t >> b) & 1); });
            if (counts) {
                sum_all += sym;
                if (q.considered[j]) sum_con += sym;
            }
        }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum_all += __shfl_xor(sum_all, d, 64);
        sum_con += __shfl_xor(sum_con, d, 64);
    }
    if (lane == 0) {
        red[w][0] = sum_all;
        red[w][1] = sum_con;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int nb = (a.R / 64) * ntile;
        const size_t slot = ((size_t)(sc * q.nst + st) * nb + (size_t)(rl0 / 64) * ntile + tile);
        const int k = threadIdx.x;
        q.part[slot * 2 + k] = (((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) / M_LN2;
    }
}

// one thread per (SNR point of the chunk, stage, edge class): its nb slots in slot order
__global__ void __launch_bounds__(64) k_llr_info_sum(LlrInfoK q, int nb, int n) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int k = i & 1, st = (i >> 1) % q.nst, sc = (i >> 1) / q.nst;
    const double* p = q.part + (size_t)(i >> 1) * nb * 2 + k;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += p[2 * b];
    const int stage = q.st_lo + st, snr = q.k.snr0 + sc;
    double* dst = stage < q.k.S ? q.acc_est + ((size_t)snr * q.k.S + stage) * 2 + k : q.acc_perf + (size_t)snr * 2 + k;
    *dst += s;
}

void launch_llr_info(hipStream_t s, const LlrInfoK& a) {
    if (a.nst <= 0) return;
    const int ntile = (a.k.ND + LLR_INFO_LT - 1) / LLR_INFO_LT;
    hipLaunchKernelGGL(k_llr_info, dim3(a.k.U / 64, a.nst * ntile), dim3(256), 0, s, a);
    const int n = (a.k.U / a.k.R) * a.nst * 2;
    hipLaunchKernelGGL(k_llr_info_sum, dim3((n + 63) / 64), dim3(64), 0, s, a, (a.k.R / 64) * ntile, n);
}

// k_llr_calib — the demapper noise ratio per data symbol, summed over the
// realisations.  Phase 1 is k_llr_info's (llr_input; lane = unit, element-major
// reads, pseudo-stage S from h[l][rep]); in place of llr_demap one lookup of the
// transmitted symbol and c |e|^2 / pn_eff.  The sum runs over the lanes and
// stays per symbol, so a block owns (SNR point, stage, tile of LLR_CALIB_LT
// symbols) and its waves walk the SNR point's R / 64 unit waves themselves: the
// per-lane sums live in registers (LLR_CALIB_LT / 4 per lane, statically
// indexed), one butterfly per symbol at the end, and lane 0 adds the result to
// the call's device accumulator, which no other block of the launch touches.
__global__ void __launch_bounds__(256) k_llr_calib(LlrCalibK q) {
    constexpr int LT = LLR_CALIB_LT, PER = LT / 4;
    const LlrK& a = q.k;
    const int ntile = (a.ND + LT - 1) / LT;
    const int st = blockIdx.y / ntile, e0 = (blockIdx.y % ntile) * LT;
    const int stage = q.st_lo + st;
    const bool pseudo = stage == a.S;                      // the perfect-CSI one-tap receiver
    const int sc = blockIdx.x, snr = a.snr0 + sc;          // SNR point of the chunk
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t U = (size_t)a.U;
    const LlrSrc sr = llr_src(a, stage);
    const double pnk = a.pn[snr];
    const double c = a.real_detect ? 2.0 : 1.0;            // a real observation has variance pn_eff / 2
    double sum[PER];
#pragma unroll
    for (int i = 0; i < PER; ++i) sum[i] = 0.0;
    for (int rl0 = 0; rl0 < a.rvalid; rl0 += 64) {         // the SNR point's unit waves, in order
        const int rep = rl0 + lane;
        const bool counts = rep < a.rvalid;                // a padding realisation adds nothing
        const size_t unit = (size_t)sc * a.R + rep;
        const size_t hunit = sr.perf ? (size_t)rep : unit;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int j = e0 + w + 4 * i;
            if (j >= a.ND) break;                          // wave-uniform
            double2 x;
            double pe;
            llr_input(a, sr.y, sr.base, U, unit, sr.h, sr.hbase, sr.hU, hunit, j, pnk, x, pe);
            const unsigned t = counts ? q.sidx[(size_t)j * a.R + rep] : 0u;
            const double2 s = a.tab.symbols[t];
            const double dx = x.x - s.x, dy = a.real_detect ? 0.0 : x.y - s.y;
            const double r = c * (dx * dx + dy * dy) / pe;
            if (counts) sum[i] += r;
        }
    }
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        double v = sum[i];
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
        const int j = e0 + w + 4 * i;
        if (lane == 0 && j < a.ND) {
            double* dst = pseudo ? q.acc_perf + (size_t)snr * a.ND + j : q.acc_est + ((size_t)snr * a.S + stage) * a.ND + j;
            *dst += v;
        }
    }
}

void launch_llr_calib(hipStream_t s, const LlrCalibK& a) {
    if (a.nst <= 0) return;
    const int ntile = (a.k.ND + LLR_CALIB_LT - 1) / LLR_CALIB_LT;
    hipLaunchKernelGGL(k_llr_calib, dim3(a.k.U / a.k.R, a.nst * ntile), dim3(256), 0, s, a);
}

}  // namespace dsce
