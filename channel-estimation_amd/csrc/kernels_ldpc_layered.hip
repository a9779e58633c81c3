// kernels_ldpc_layered.hip — the layered normalised min-sum LDPC decoder of
// include/dsce.h (DSCE_HAS_LDPC_LAYERED): k_ldpc_layered (dsce_run_ldpc_layered)
// decodes the LLRs of k_llr, signed against the transmitted bits, and counts the
// decoded ones; k_ldpc_layered_probe (dsce_ldpc_layered) decodes the caller's lam
// and stores every decided bit.  One device function, ldpc_layered_block, serves
// both, with a load callback.
//
// One workgroup per codeword, everything of the codeword in dynamic LDS as in
// kernels_ldpc.hip: P [N] fp64 and one 24-byte record (m1, m2, sign mask, i1, sg)
// per check, from which R_{c,p} = +-alpha (p == i1 ? m2 : m1) is recomputed where
// it is read.  The layers of an iteration run in order, a barrier after each.
// Inside a layer lane = edge: the checks of a layer share no variable, so a lane
// owns its P_v, reads it once and writes it in place.  The host lays the lanes of
// a layer out (LdpcLayersK): each check takes a group of 2^lg >= degree
// consecutive lanes, aligned to its size and therefore inside one wave, the
// groups of a layer in descending size; lanes past the degree and the lanes that
// fill the layer up to a multiple of 64 carry variable -1, that is a = +inf, s = 0.
// The record (m1, i1, m2, mask) of a group is formed by a butterfly over its lg
// steps (DPP moves inside a row of 16 lanes, below), every lane ending with the
// whole record: the minimum is exact, "the lowest position among equal
// minima" is the lexicographic minimum of (a, p), and
// m2 of two halves is min(m2 of the half that holds i1, m1 of the other), so any
// tree gives the defined bits.  The lane of position 0 stores the record; the
// other lanes of the group (the same wave) have read the old one before.  A layer
// wider than the workgroup is walked in strides of blockDim, with no barrier in
// between.
// The syndrome of x = (P < 0) after the last layer is a read-only pass, thread =
// check, with the block-uniform exit over two alternating LDS flag words of
// k_ldpc; without early_stop the pass and its barrier are not run.
// fp64 in the order of include/dsce.h, no FMA (-ffp-contract=off), no clipping.
#include "dsce_dispatch.h"
#include "dsce_kernels.h"

#include <math.h>

namespace dsce {

// The same bytes as k_ldpc's LDS in another order: the records first, so that (m1, m2) is one aligned 16-byte
// read and (mask, i1 | sg << 8) one 8-byte read, then P, then the flag words.
struct LayeredLds {
    double2* mm;              // [M] (m1, m2)
    uint2* si;                // [M] (sign mask, i1 | sg << 8)
    double* P;                // [N]
    int* flag;                // [2]
};

__device__ __forceinline__ LayeredLds layered_carve(unsigned char* base, int N, int M) {
    LayeredLds l;
    l.mm = (double2*)base;
    l.si = (uint2*)(l.mm + M);
    l.P = (double*)(l.si + M);
    l.flag = (int*)(l.P + N);
    return l;
}

// the message of edge position p from a check's record (ldpc_msg of kernels_ldpc.hip)
__device__ __forceinline__ double ldpc_record_msg(double2 mm, uint2 si, int p, double alpha) {
    const double r = alpha * (p == (int)(si.y & 0xFFu) ? mm.y : mm.x);
    return (((si.y >> 8) ^ (si.x >> p)) & 1u) ? -r : r;
}

// The record of one side of a butterfly step, and the exchange with the other side.  After the steps below k
// every lane of an aligned group of 2^k holds that group's record, so any lane of the sibling group will do:
// steps 0 and 1 swap inside a quad (quad_perm), step 2 mirrors the 8 lanes and step 3 the 16 lanes of a DPP row
// (row_half_mirror, row_mirror): VALU moves, no LDS traffic.  Only step 4 (a check of more than 16 variables)
// crosses rows, by __shfl_xor.
struct LayeredRec {
    double m1, m2;
    int i1;
    unsigned mask;
};
constexpr int DPP_QUAD_XOR1 = 0xB1, DPP_QUAD_XOR2 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140;
template <int CTRL>
__device__ __forceinline__ int layered_dpp(int x) {
    return __builtin_amdgcn_update_dpp(0, x, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ double layered_dpp(double x) {
    return __hiloint2double(layered_dpp<CTRL>(__double2hiint(x)), layered_dpp<CTRL>(__double2loint(x)));
}
template <int CTRL>
__device__ __forceinline__ LayeredRec layered_other(const LayeredRec& r) {
    LayeredRec o;
    if constexpr (CTRL < 0) {
        o.m1 = __shfl_xor(r.m1, 16);
        o.m2 = __shfl_xor(r.m2, 16);
        o.i1 = __shfl_xor(r.i1, 16);
        o.mask = (unsigned)__shfl_xor((int)r.mask, 16);
    } else {
        o.m1 = layered_dpp<CTRL>(r.m1);
        o.m2 = layered_dpp<CTRL>(r.m2);
        o.i1 = layered_dpp<CTRL>(r.i1);
        o.mask = (unsigned)layered_dpp<CTRL>((int)r.mask);
    }
    return o;
}
// two halves into one, the same on both sides: the lexicographic minimum of (m1, i1), m2 = min(m2 of the half that
// holds it, m1 of the other)
__device__ __forceinline__ void layered_merge(LayeredRec& r, const LayeredRec& o, bool on) {
    if (!on) return;
    if (o.m1 < r.m1 || (o.m1 == r.m1 && o.i1 < r.i1)) {
        r.m2 = fmin(o.m2, r.m1);
        r.m1 = o.m1;
        r.i1 = o.i1;
    } else {
        r.m2 = fmin(r.m2, o.m1);
    }
    r.mask |= o.mask;
}

// load(v) -> ell_v of a variable v < N (0.0 for slot -1).  Returns the iterations
// performed; on return P holds the last iteration's sums, visible to every thread.
template <class Load>
__device__ __forceinline__ int ldpc_layered_block(const LdpcCodeK& c, const LdpcLayersK& y, const LayeredLds& l, Load load) {
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int v = tid; v < c.N; v += nt) l.P[v] = load(v);
    for (int ch = tid; ch < c.M; ch += nt) {               // R = +0.0 on every edge
        l.mm[ch] = make_double2(0.0, 0.0);
        l.si[ch] = make_uint2(0u, 0u);
    }
    if (tid < 2) l.flag[tid] = 0;
    __syncthreads();
    int it = 0;
    for (;;) {
        for (int ly = 0; ly < y.n_layers; ++ly) {
            // lane_ptr and blockDim are multiples of 64: a wave is in the loop whole or not at all
            const int end = y.lane_ptr[ly + 1];
            for (int i = y.lane_ptr[ly] + tid; i < end; i += nt) {
                const int2 w = y.lane[i];
                const int v = w.x, ch = w.y >> 8, p = (w.y >> 3) & 31, lg = w.y & 7;
                double q = 0.0;
                LayeredRec r{INFINITY, INFINITY, p, 0u};
                if (v >= 0) {
                    q = l.P[v] - ldpc_record_msg(l.mm[ch], l.si[ch], p, c.alpha);
                    r.m1 = fabs(q);
                    r.mask = (q < 0.0 ? 1u : 0u) << p;
                }
                // the groups of a layer descend in size: the wave's first lane has its largest
                const int steps = __builtin_amdgcn_readfirstlane(lg);
                if (steps > 0) layered_merge(r, layered_other<DPP_QUAD_XOR1>(r), lg > 0);
                if (steps > 1) layered_merge(r, layered_other<DPP_QUAD_XOR2>(r), lg > 1);
                if (steps > 2) layered_merge(r, layered_other<DPP_ROW_HALF_MIRROR>(r), lg > 2);
                if (steps > 3) layered_merge(r, layered_other<DPP_ROW_MIRROR>(r), lg > 3);
                if (steps > 4) layered_merge(r, layered_other<-1>(r), lg > 4);
                if (v >= 0) {
                    const unsigned sg = __popc(r.mask) & 1u;
                    const double x = c.alpha * (p == r.i1 ? r.m2 : r.m1);
                    l.P[v] = q + (((sg ^ (r.mask >> p)) & 1u) ? -x : x);
                    if (p == 0) {
                        l.mm[ch] = make_double2(r.m1, r.m2);
                        l.si[ch] = make_uint2(r.mask, (unsigned)r.i1 | (sg << 8));
                    }
                }
            }
            __syncthreads();
        }
        ++it;
        if (c.early_stop) {
            bool odd = false;
            for (int ch = tid; ch < c.M; ch += nt) {
                unsigned syn = 0u;
                const int e1 = c.row_ptr[ch + 1];
                for (int e = c.row_ptr[ch]; e < e1; ++e) syn ^= l.P[c.col[e]] < 0.0 ? 1u : 0u;
                odd |= syn != 0u;
            }
            if (odd) l.flag[it & 1] = 1;
            __syncthreads();
            const bool done = l.flag[it & 1] == 0;         // x of iteration `it` satisfies every check
            if (tid == 0) l.flag[(it + 1) & 1] = 0;        // last read before the layers' barriers
            if (done) break;
        }
        if (it >= c.max_iter) break;
    }
    __syncthreads();                                       // the flag words are free for the callers
    return it;
}

// k_ldpc_layered — one block per codeword of q.cw (CodewordK: placement, lam, counts), ell = -lam.
__global__ void __launch_bounds__(1024) k_ldpc_layered(LdpcLayeredK q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char layered_lds[];
    const LayeredLds l = layered_carve(layered_lds, q.c.N, q.c.M);
    const CodewordAt at = codeword_at(q.cw, blockIdx.x);
    const int it = ldpc_layered_block(q.c, q.y, l, [&](int v) {
        const int slot = q.c.slot[v];
        return slot < 0 ? 0.0 : -codeword_lam(q.cw, at, slot);
    });
    int errs = 0;
    for (int v = threadIdx.x; v < q.c.n_info; v += blockDim.x) errs += l.P[v] < 0.0 ? 1 : 0;
    if (threadIdx.x == 0) l.flag[0] = 0;
    __syncthreads();
    if (errs) atomicAdd(l.flag, errs);
    __syncthreads();
    if (threadIdx.x == 0) {
        codeword_count(q.cw, at, l.flag[0]);
        if (q.acc_iter) atomicAdd(q.acc_iter + at.cell, (unsigned long long)it);
    }
}

// k_ldpc_layered_probe — the same decoder on the caller's lam [ncw][n_slots]; x goes
// to bits [ncw][N] and the iterations performed to iters [ncw].
__global__ void __launch_bounds__(1024) k_ldpc_layered_probe(LdpcCodeK c, LdpcLayersK y, long long n_slots,
                                                              const double* __restrict__ lam, uint8_t* __restrict__ bits,
                                                              int* __restrict__ iters) {
    extern __shared__ __attribute__((aligned(16))) unsigned char layered_lds[];
    const LayeredLds l = layered_carve(layered_lds, c.N, c.M);
    const double* src = lam + (size_t)blockIdx.x * (size_t)n_slots;
    const int it = ldpc_layered_block(c, y, l, [&](int v) {
        const int slot = c.slot[v];
        return slot < 0 ? 0.0 : -src[slot];
    });
    uint8_t* o = bits + (size_t)blockIdx.x * (size_t)c.N;
    for (int v = threadIdx.x; v < c.N; v += blockDim.x) o[v] = l.P[v] < 0.0 ? 1 : 0;
    if (iters && threadIdx.x == 0) iters[blockIdx.x] = it;
}

// dynamic LDS past 64 KiB has to be announced per kernel
template <class K>
static void layered_lds_attr(K kernel, size_t lds) {
    if (lds <= 64 * 1024) return;
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess)
        throw std::runtime_error(std::string("k_ldpc_layered: hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") +
                                 hipGetErrorString(e));
}

void launch_ldpc_layered(hipStream_t s, const LdpcLayeredK& a) {
    if (a.cw.ncw <= 0) return;
    const size_t lds = ldpc_layered_lds_bytes(a.c.N, a.c.M);
    layered_lds_attr(k_ldpc_layered, lds);
    hipLaunchKernelGGL(k_ldpc_layered, dim3((unsigned)a.cw.ncw), dim3(a.y.threads), lds, s, a);
}

void launch_ldpc_layered_probe(hipStream_t s, const LdpcCodeK& c, const LdpcLayersK& y, long long ncw, long long n_slots,
                               const double* lam, uint8_t* bits, int* iters) {
    if (ncw <= 0) return;
    const size_t lds = ldpc_layered_lds_bytes(c.N, c.M);
    layered_lds_attr(k_ldpc_layered_probe, lds);
    hipLaunchKernelGGL(k_ldpc_layered_probe, dim3((unsigned)ncw), dim3(y.threads), lds, s, c, y, n_slots, lam, bits, iters);
}

}  // namespace dsce
