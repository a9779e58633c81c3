// kernels_ldpc_fixed.hip — the fixed-point min-sum LDPC decoder of include/dsce.h
// (DSCE_HAS_LDPC_FIXED): k_ldpc_fixed (dsce_run_ldpc_fixed) decodes the LLRs of
// k_llr, signed against the transmitted bits and the caller's codeword, and counts
// the decoded bits that differ from it; k_ldpc_fixed_probe (dsce_ldpc_fixed)
// decodes the caller's lam and stores every decided bit and, on request, every
// final P_v.  One device function, ldpc_fixed_block, serves both, with a load
// callback that returns the quantised ell_v: the quantiser in the prologue is the
// only floating point of the kernel.
//
// One workgroup per codeword, flooding schedule, k_ldpc's phases, barriers and
// syndrome flags (kernels_ldpc.hip), everything of the codeword in dynamic LDS as
// 16- and 32-bit integers: two flag words, one 8-byte record per check (r1 | r2 <<
// 16, the sign mask), i1 | sg << 8 per check as 16 bits, then P [N] and ell [N] as
// int16: 4 N + 10 M + 8 bytes.  r1 and r2 are m1 and m2 AFTER the normalisation and
// the offset, r = max(((mu alpha_num + half) >> alpha_shift) - beta, 0), formed
// once per check where the record is written; R_{c,p} = +-(p == i1 ? r2 : r1) is
// then a select and a sign where it is read: the same integers as a stored message.
// ell lives in LDS, not in registers, so one instance serves every N and every
// workgroup size.
#include "dsce_dispatch.h"
#include "dsce_kernels.h"

#include <math.h>

#ifndef DSCE_LDPC_FIXED_MAX_THREADS
// The cap on threads per block, also the kernels' launch bound.  Measured at N = 2560 (ns per
// codeword and iteration at rates 1/2 and 3/4): 128: 15.0, 12.3; 256: 9.4, 9.8; 512: 9.0, 10.5; 1024: 9.9, 11.4.
#define DSCE_LDPC_FIXED_MAX_THREADS 256
#endif
static_assert(DSCE_LDPC_FIXED_MAX_THREADS >= 64 && DSCE_LDPC_FIXED_MAX_THREADS <= 1024 && DSCE_LDPC_FIXED_MAX_THREADS % 64 == 0,
              "whole waves, at most 1024 threads");

namespace dsce {

struct LdpcFixedLds {
    int* flag;                // [2]
    uint2* rec;               // [M] x = r1 | r2 << 16, y = sign mask
    unsigned short* info;     // [M] i1 | sg << 8
    short* P;                 // [N]
    short* ell;               // [N]
};

__device__ __forceinline__ LdpcFixedLds ldpc_fixed_carve(unsigned char* base, int N, int M) {
    LdpcFixedLds l;
    l.flag = (int*)base;
    l.rec = (uint2*)(base + 8);
    l.info = (unsigned short*)(l.rec + M);
    l.P = (short*)(l.info + M);
    l.ell = l.P + N;
    return l;
}

// step 1 of the header: round half away from zero, saturate at C; NaN gives 0.  What
// is converted to int is an integer-valued double in [0, C].
__device__ __forceinline__ int ldpc_fixed_quantise(double lam, const LdpcFixedParK& f) {
    const double t = (-lam) * f.scale;
    const double a = fabs(t);
    if (!(a == a)) return 0;
    const double cap = (double)f.C;
    const int mag = (int)(a >= cap ? cap : floor(a + 0.5));
    return t < 0.0 ? -mag : mag;
}

// the message of edge position p from a check's record
__device__ __forceinline__ int ldpc_fixed_msg(uint2 rec, unsigned info, int p) {
    const int r = p == (int)(info & 0xFFu) ? (int)(rec.x >> 16) : (int)(rec.x & 0xFFFFu);
    return (((info >> 8) ^ (rec.y >> p)) & 1u) ? -r : r;
}

__device__ __forceinline__ int ldpc_fixed_clamp(int v, int lim) { return min(max(v, -lim), lim); }

// load(v) -> ell_v of a variable v < N.  Returns the iterations performed; on return
// P holds the last iteration's sums, visible to every thread.
template <class Load>
__device__ __forceinline__ int ldpc_fixed_block(const LdpcCodeK& c, const LdpcFixedParK& f, const LdpcFixedLds& l,
                                                Load load) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int v = tid; v < c.N; v += nt) {
        const short e = (short)load(v);
        l.ell[v] = e;
        l.P[v] = e;
    }
    for (int ch = tid; ch < c.M; ch += nt) {               // R = 0 on every edge
        l.rec[ch] = make_uint2(0u, 0u);
        l.info[ch] = 0;
    }
    if (tid < 2) l.flag[tid] = 0;
    __syncthreads();
    int it = 0;
    for (;;) {
        int* flag = l.flag + (it & 1);
        bool odd = false;
        for (int ch = tid; ch < c.M; ch += nt) {
            const int e0 = c.row_ptr[ch], d = c.row_ptr[ch + 1] - e0;
            const uint2 orec = l.rec[ch];
            const unsigned oinfo = l.info[ch];
            int m1 = 0x7FFFFFFF, m2 = 0x7FFFFFFF;
            unsigned mask = 0u, i1 = 0u, syn = 0u;
            for (int p = 0; p < d; ++p) {
                const int Pv = l.P[c.col[e0 + p]];
                syn ^= Pv < 0 ? 1u : 0u;
                const int q = ldpc_fixed_clamp(Pv - ldpc_fixed_msg(orec, oinfo, p), f.X);
                const int a = abs(q);
                mask |= (q < 0 ? 1u : 0u) << p;
                if (a < m1) {                              // the lowest position attaining the minimum
                    m2 = m1;
                    m1 = a;
                    i1 = (unsigned)p;
                } else if (a < m2) {
                    m2 = a;
                }
            }
            // d >= 2, so m1 <= m2 <= X < 2^15 here
            const int r1 = max(((m1 * f.an + f.half) >> f.sh) - f.beta, 0);
            const int r2 = max(((m2 * f.an + f.half) >> f.sh) - f.beta, 0);
            l.rec[ch] = make_uint2((unsigned)r1 | ((unsigned)r2 << 16), mask);
            l.info[ch] = (unsigned short)(i1 | ((__popc(mask) & 1u) << 8));
            odd |= syn != 0u;
        }
        if (c.early_stop && it > 0 && odd) *flag = 1;
        __syncthreads();
        if (c.early_stop && it > 0 && *flag == 0) break;   // x of iteration `it` satisfies every check
        if (tid == 0) l.flag[(it + 1) & 1] = 0;            // last read before the previous barrier
        for (int v = tid; v < c.N; v += nt) {
            int acc = l.ell[v];
            const int e1 = c.vptr[v + 1];
            for (int e = c.vptr[v]; e < e1; ++e) {
                const int pk = c.vedge[e], ch = pk >> 5;
                acc += ldpc_fixed_msg(l.rec[ch], l.info[ch], pk & 31);
            }
            l.P[v] = (short)ldpc_fixed_clamp(acc, f.A);
        }
        ++it;
        __syncthreads();
        if (it >= c.max_iter) break;
    }
    return it;
}

// k_ldpc_fixed — one block per codeword of q.cw (CodewordK: placement, lam, counts); ell0 = Q(-lam), negated where
// the caller's codeword has a 1, and the decided bits are counted against that word.
__global__ void __launch_bounds__(DSCE_LDPC_FIXED_MAX_THREADS) k_ldpc_fixed(LdpcFixedK q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_fixed_lds[];
    const LdpcFixedLds l = ldpc_fixed_carve(ldpc_fixed_lds, q.c.N, q.c.M);
    const CodewordAt at = codeword_at(q.cw, blockIdx.x);
    const int it = ldpc_fixed_block(q.c, q.f, l, [&](int v) {
        const int slot = q.c.slot[v];
        const int e = slot < 0 ? 0 : ldpc_fixed_quantise(codeword_lam(q.cw, at, slot), q.f);
        return q.word && q.word[v] ? -e : e;
    });
    int errs = 0;
    for (int v = threadIdx.x; v < q.c.n_info; v += blockDim.x) {
        const int cv = q.word ? (int)q.word[v] : 0;
        errs += (l.P[v] < 0 ? 1 : 0) ^ cv;
    }
    // flag[0] is free now.  Leaving at max_iter, every thread has passed the barrier after the last read of a flag.
    // Leaving at the early stop of iteration `it`, the threads have read flag[it & 1] == 0 with no barrier after that
    // read, so thread 0's store can overtake another thread's read: if the word is flag[0], the store writes the 0
    // that is there and the read sees 0 either way; if it is flag[1], nobody reads flag[0] any more.
    if (threadIdx.x == 0) l.flag[0] = 0;
    __syncthreads();
    if (errs) atomicAdd(l.flag, errs);
    __syncthreads();
    if (threadIdx.x == 0) {
        codeword_count(q.cw, at, l.flag[0]);
        if (q.acc_iter) atomicAdd(q.acc_iter + at.cell, (unsigned long long)it);
    }
}

// k_ldpc_fixed_probe — the same decoder on the caller's lam [ncw][n_slots]; x goes to bits [ncw][N], the iterations
// performed to iters [ncw] and the final P to app [ncw][N] (each of the last two or null).
__global__ void __launch_bounds__(DSCE_LDPC_FIXED_MAX_THREADS) k_ldpc_fixed_probe(LdpcCodeK c, LdpcFixedParK f, long long n_slots,
                                                            const double* __restrict__ lam, uint8_t* __restrict__ bits,
                                                            int* __restrict__ iters, short* __restrict__ app) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_fixed_lds[];
    const LdpcFixedLds l = ldpc_fixed_carve(ldpc_fixed_lds, c.N, c.M);
    const double* src = lam + (size_t)blockIdx.x * (size_t)n_slots;
    const int it = ldpc_fixed_block(c, f, l, [&](int v) {
        const int slot = c.slot[v];
        return slot < 0 ? 0 : ldpc_fixed_quantise(src[slot], f);
    });
    uint8_t* o = bits + (size_t)blockIdx.x * (size_t)c.N;
    for (int v = threadIdx.x; v < c.N; v += blockDim.x) o[v] = l.P[v] < 0 ? 1 : 0;
    if (app) {
        short* a = app + (size_t)blockIdx.x * (size_t)c.N;
        for (int v = threadIdx.x; v < c.N; v += blockDim.x) a[v] = l.P[v];
    }
    if (iters && threadIdx.x == 0) iters[blockIdx.x] = it;
}

// threads per block: whole waves up to the cap; beyond it both phases stride
static int ldpc_fixed_threads(const LdpcCodeK& c) {
    return std::min(DSCE_LDPC_FIXED_MAX_THREADS, (std::max(c.N, c.M) + 63) / 64 * 64);
}

// dynamic LDS past 64 KiB has to be announced per kernel
template <class K>
static void ldpc_fixed_lds_attr(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
        throw std::runtime_error(std::string("k_ldpc_fixed: hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") +
                                 hipGetErrorString(e));
}

void launch_ldpc_fixed(hipStream_t s, const LdpcFixedK& a) {
    if (a.cw.ncw <= 0) return;
    const size_t lds = ldpc_fixed_lds_bytes(a.c.N, a.c.M);
    ldpc_fixed_lds_attr(k_ldpc_fixed, lds);
    hipLaunchKernelGGL(k_ldpc_fixed, dim3((unsigned)a.cw.ncw), dim3(ldpc_fixed_threads(a.c)), lds, s, a);
}

void launch_ldpc_fixed_probe(hipStream_t s, const LdpcCodeK& c, const LdpcFixedParK& f, long long ncw, long long n_slots,
                             const double* lam, uint8_t* bits, int* iters, short* app) {
    if (ncw <= 0) return;
    const size_t lds = ldpc_fixed_lds_bytes(c.N, c.M);
    ldpc_fixed_lds_attr(k_ldpc_fixed_probe, lds);
    hipLaunchKernelGGL(k_ldpc_fixed_probe, dim3((unsigned)ncw), dim3(ldpc_fixed_threads(c)), lds, s, c, f, n_slots, lam,
                       bits, iters, app);
}

}  // namespace dsce
