// kernels_ldpc.hip — the normalised min-sum LDPC decoder of include/dsce.h
// (DSCE_HAS_LDPC_RUN): k_ldpc (dsce_run_ldpc) decodes the LLRs of k_llr, signed
// against the transmitted bits, and counts the decoded ones; k_ldpc_probe
// (dsce_ldpc) decodes the caller's lam and stores every decided bit.  One device
// function, ldpc_block, serves both, with a load callback.
//
// One workgroup per codeword, flooding schedule, everything of the codeword in
// dynamic LDS: P [N] fp64 and one 24-byte record (m1, m2, sign mask, i1, sg) per
// check, from which R_{c,p} = +-alpha (p == i1 ? m2 : m1) is recomputed where it
// is read: the same bits as a stored message.  An iteration is
//   check phase    thread = check (stride blockDim): q_p = P_v - R_{c,p} over the
//                  check's <= 32 edges, the new record in registers, stored over
//                  the old one (only this thread reads it in this phase);
//   barrier
//   variable phase thread = variable tid + k blockDim, k < VPT: ell from a
//                  register (VPT = 0, beyond 16 variables per thread: read again
//                  through L2), the new messages in ascending check order
//                  through the variable-major adjacency, P'_v stored;
//   barrier.
// The syndrome of x = (P < 0) after iteration i is taken by the check phase of
// iteration i + 1, which reads those P anyway: a thread that sees an unsatisfied
// check raises one of two alternating LDS flag words, and every thread reads it
// after the barrier, so the exit is block-uniform and costs one check phase.
// fp64 in the order of include/dsce.h, no FMA (-ffp-contract=off), no clipping.
#include "dsce_dispatch.h"
#include "dsce_kernels.h"

#include <math.h>

namespace dsce {

struct LdpcLds {
    double* P;
    double* m1;
    double* m2;
    unsigned* mask;
    unsigned* info;           // i1 | sg << 8
    int* flag;                // [2]
};

__device__ __forceinline__ LdpcLds ldpc_carve(unsigned char* base, int N, int M) {
    LdpcLds l;
    l.P = (double*)base;
    l.m1 = l.P + N;
    l.m2 = l.m1 + M;
    l.mask = (unsigned*)(l.m2 + M);
    l.info = l.mask + M;
    l.flag = (int*)(l.info + M);
    return l;
}

// the message of edge position p from a check's record
__device__ __forceinline__ double ldpc_msg(double m1, double m2, unsigned mask, unsigned info, int p, double alpha) {
    const double r = alpha * (p == (int)(info & 0xFFu) ? m2 : m1);
    return (((info >> 8) ^ (mask >> p)) & 1u) ? -r : r;
}

// load(v) -> ell_v of a variable v < N (0.0 for slot -1).  Returns the iterations
// performed; on return P holds the last iteration's sums, visible to every thread.
template <int VPT, class Load>
__device__ __forceinline__ int ldpc_block(const LdpcCodeK& c, const LdpcLds& l, Load load) {
    const int tid = threadIdx.x, nt = blockDim.x;
    double ell[VPT ? VPT : 1];
    if constexpr (VPT > 0) {
#pragma unroll
        for (int k = 0; k < VPT; ++k) {
            const int v = tid + k * nt;
            ell[k] = 0.0;
            if (v < c.N) {
                ell[k] = load(v);
                l.P[v] = ell[k];
            }
        }
    } else {
        for (int v = tid; v < c.N; v += nt) l.P[v] = load(v);
    }
    // P'_v of one variable from the records of its checks
    auto update = [&](int v, double acc) {
        const int e1 = c.vptr[v + 1];
        for (int e = c.vptr[v]; e < e1; ++e) {
            const int pk = c.vedge[e], ch = pk >> 5;
            acc += ldpc_msg(l.m1[ch], l.m2[ch], l.mask[ch], l.info[ch], pk & 31, c.alpha);
        }
        l.P[v] = acc;
    };
    for (int ch = tid; ch < c.M; ch += nt) {               // R = +0.0 on every edge
        l.m1[ch] = 0.0;
        l.m2[ch] = 0.0;
        l.mask[ch] = 0u;
        l.info[ch] = 0u;
    }
    if (tid < 2) l.flag[tid] = 0;
    __syncthreads();
    int it = 0;
    for (;;) {
        int* flag = l.flag + (it & 1);
        bool odd = false;
        for (int ch = tid; ch < c.M; ch += nt) {
            const int e0 = c.row_ptr[ch], d = c.row_ptr[ch + 1] - e0;
            const double o1 = l.m1[ch], o2 = l.m2[ch];
            const unsigned omask = l.mask[ch], oinfo = l.info[ch];
            double m1 = INFINITY, m2 = INFINITY;
            unsigned mask = 0u, i1 = 0u, syn = 0u;
            for (int p = 0; p < d; ++p) {
                const double Pv = l.P[c.col[e0 + p]];
                syn ^= Pv < 0.0 ? 1u : 0u;
                const double q = Pv - ldpc_msg(o1, o2, omask, oinfo, p, c.alpha);
                const double a = fabs(q);
                mask |= (q < 0.0 ? 1u : 0u) << p;
                if (a < m1) {                              // the lowest position attaining the minimum
                    m2 = m1;
                    m1 = a;
                    i1 = (unsigned)p;
                } else if (a < m2) {
                    m2 = a;
                }
            }
            l.m1[ch] = m1;
            l.m2[ch] = m2;
            l.mask[ch] = mask;
            l.info[ch] = i1 | ((__popc(mask) & 1u) << 8);
            odd |= syn != 0u;
        }
        if (c.early_stop && it > 0 && odd) *flag = 1;
        __syncthreads();
        if (c.early_stop && it > 0 && *flag == 0) break;   // x of iteration `it` satisfies every check
        if (tid == 0) l.flag[(it + 1) & 1] = 0;            // last read before the previous barrier
        if constexpr (VPT > 0) {
#pragma unroll
            for (int k = 0; k < VPT; ++k) {
                const int v = tid + k * nt;
                if (v < c.N) update(v, ell[k]);
            }
        } else {
            for (int v = tid; v < c.N; v += nt) update(v, load(v));
        }
        ++it;
        __syncthreads();
        if (it >= c.max_iter) break;
    }
    return it;
}

// k_ldpc — one block per codeword of q.cw (CodewordK: placement, lam, counts), ell = -lam.
template <int VPT>
__global__ void __launch_bounds__(1024) k_ldpc(LdpcK q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_lds[];
    const LdpcLds l = ldpc_carve(ldpc_lds, q.c.N, q.c.M);
    const CodewordAt at = codeword_at(q.cw, blockIdx.x);
    const int it = ldpc_block<VPT>(q.c, l, [&](int v) {
        const int slot = q.c.slot[v];
        return slot < 0 ? 0.0 : -codeword_lam(q.cw, at, slot);
    });
    int errs = 0;
    for (int v = threadIdx.x; v < q.c.n_info; v += blockDim.x) errs += l.P[v] < 0.0 ? 1 : 0;
    // flag[0] and flag[1] are free now: every thread left the loop behind a barrier
    if (threadIdx.x == 0) l.flag[0] = 0;
    __syncthreads();
    if (errs) atomicAdd(l.flag, errs);
    __syncthreads();
    if (threadIdx.x == 0) {
        codeword_count(q.cw, at, l.flag[0]);
        if (q.acc_iter) atomicAdd(q.acc_iter + at.cell, (unsigned long long)it);
    }
}

// k_ldpc_probe — the same decoder on the caller's lam [ncw][n_slots]; x goes to
// bits [ncw][N] and the iterations performed to iters [ncw].
template <int VPT>
__global__ void __launch_bounds__(1024) k_ldpc_probe(LdpcCodeK c, long long n_slots, const double* __restrict__ lam,
                                                      uint8_t* __restrict__ bits, int* __restrict__ iters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_lds[];
    const LdpcLds l = ldpc_carve(ldpc_lds, c.N, c.M);
    const double* src = lam + (size_t)blockIdx.x * (size_t)n_slots;
    const int it = ldpc_block<VPT>(c, l, [&](int v) {
        const int slot = c.slot[v];
        return slot < 0 ? 0.0 : -src[slot];
    });
    uint8_t* o = bits + (size_t)blockIdx.x * (size_t)c.N;
    for (int v = threadIdx.x; v < c.N; v += blockDim.x) o[v] = l.P[v] < 0.0 ? 1 : 0;
    if (iters && threadIdx.x == 0) iters[blockIdx.x] = it;
}

// threads per block: a thread per variable / check up to 1024; then VPT variables per thread
static int ldpc_threads(const LdpcCodeK& c) { return std::min(1024, (std::max(c.N, c.M) + 63) / 64 * 64); }

// dynamic LDS past 64 KiB has to be announced per kernel
template <class K>
static void ldpc_lds_attr(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
        throw std::runtime_error(std::string("k_ldpc: hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") +
                                 hipGetErrorString(e));
}

// the instance whose VPT covers ceil(N / threads): 1, 2, 4, 8, 16 registers of ell, 0 = ell read again
static int ldpc_vpt(const LdpcCodeK& c, int nt) {
    const int need = (c.N + nt - 1) / nt;
    for (int v : {1, 2, 4, 8, 16})
        if (need <= v) return v;
    return 0;
}

void launch_ldpc(hipStream_t s, const LdpcK& a) {
    if (a.cw.ncw <= 0) return;
    const int nt = ldpc_threads(a.c);
    const size_t lds = ldpc_lds_bytes(a.c.N, a.c.M);
    for_value<1, 2, 4, 8, 16, 0>(ldpc_vpt(a.c, nt), [&](auto VPT) {
        ldpc_lds_attr(k_ldpc<VPT>, lds);
        hipLaunchKernelGGL(k_ldpc<VPT>, dim3((unsigned)a.cw.ncw), dim3(nt), lds, s, a);
    });
}

void launch_ldpc_probe(hipStream_t s, const LdpcCodeK& c, long long ncw, long long n_slots, const double* lam,
                       uint8_t* bits, int* iters) {
    if (ncw <= 0) return;
    const int nt = ldpc_threads(c);
    const size_t lds = ldpc_lds_bytes(c.N, c.M);
    for_value<1, 2, 4, 8, 16, 0>(ldpc_vpt(c, nt), [&](auto VPT) {
        ldpc_lds_attr(k_ldpc_probe<VPT>, lds);
        hipLaunchKernelGGL(k_ldpc_probe<VPT>, dim3((unsigned)ncw), dim3(nt), lds, s, c, n_slots, lam, bits, iters);
    });
}

}  // namespace dsce
