// kernels_viterbi.hip — the K = 7 Viterbi decoder of include/dsce.h
// (DSCE_HAS_CODED_RUN): k_viterbi (dsce_run_coded) decodes the LLRs of k_llr,
// signed against the transmitted bits, and counts the decoded ones;
// k_viterbi_probe (dsce_viterbi) decodes the caller's lam and stores every
// decoded input.  One device function, viterbi_wave, serves both, with a load
// and an emit callback.
//
// One wavefront per codeword, lane = next state ns (64 states).  The register
// r = (p_b << 1) | u = ns | (b << 6) holds u_t .. u_{t-6} in bits 0 .. 6, and output
// k is the parity of r & taps_k; both tap sets contain bit 6, so branch b = 1 sees
// the complement of branch b = 0's outputs and a lane keeps two flags.
//
// Forward pass, 32 trellis steps per group: lane i fetches operand i of the group
// (step t0 + i / 2, output i & 1) in one gather — src, then the callback's lam of
// that slot — and a step takes its two wave-uniform operands by lane reads.  The
// two predecessor metrics come by __shfl (four 32-bit ds_bpermute per step), the
// 64 decisions of a step are one __ballot word, written into lane t - t0 of a
// register pair (v_writelane) and stored to LDS once per group, 32 lanes x 8
// bytes: T x 8 bytes per codeword, so DSCE_CODE_MAX_STEPS = 8192
// steps fill the 64 KiB a block may use, and a block holds as many waves (<= 4)
// as fit.  No renormalisation: fp64 path metrics, in the order of include/dsce.h.
// Traceback: 64 decision words per load (lane i holds step c0 + i), walked
// wave-uniformly with lane reads; the decoded bits of the 64 steps are collected
// in one scalar word and handed to emit.  A wave touches its own LDS slice only:
// no block barrier.
#include "dsce_kernels.h"

#include <math.h>

namespace dsce {

// v_writelane_b32: `old` with lane `lane` (wave-uniform) replaced by the wave-uniform `value`.
// The compiler has the intrinsic but no builtin of that name.
__device__ int writelane(int value, int lane, int old) __asm("llvm.amdgcn.writelane.i32");

// load(slot) -> lam of a slot in [0, n_slots); emit(c0, n, bits): bit i of the
// wave-uniform `bits` is the decoded input of step c0 + i, i < n <= 64
template <class Load, class Emit>
__device__ __forceinline__ void viterbi_wave(const int* __restrict__ src, int T, int terminated,
                                             unsigned long long* dec, Load load, Emit emit) {
    const int lane = threadIdx.x & 63;
    const int p0 = lane >> 1, p1 = p0 | 32;
    const bool a0 = __popc(lane & 0x6D) & 1;               // o0 (133 octal) of branch 0: taps 0, 2, 3, 5, 6
    const bool a1 = __popc(lane & 0x4F) & 1;               // o1 (171 octal) of branch 0: taps 0, 1, 2, 3, 6
    // "o ? z : 0.0" as z & mask on the operand's two wave-uniform halves: the same bits
    const int m0 = a0 ? -1 : 0, n0 = ~m0, m1 = a1 ? -1 : 0, n1 = ~m1;
    double pm = lane == 0 ? 0.0 : -INFINITY;
    auto step = [&](int zlo, int zhi, int tt, int& wlo, int& whi) {
        const int z0l = __builtin_amdgcn_readlane(zlo, 2 * tt), z0h = __builtin_amdgcn_readlane(zhi, 2 * tt);
        const int z1l = __builtin_amdgcn_readlane(zlo, 2 * tt + 1), z1h = __builtin_amdgcn_readlane(zhi, 2 * tt + 1);
        const double q0 = __shfl(pm, p0, 64), q1 = __shfl(pm, p1, 64);
        const double c0 = (q0 + __hiloint2double(z0h & m0, z0l & m0)) + __hiloint2double(z1h & m1, z1l & m1);
        const double c1 = (q1 + __hiloint2double(z0h & n0, z0l & n0)) + __hiloint2double(z1h & n1, z1l & n1);
        const bool d = c1 > c0;                            // a tie, and -inf against -inf: b = 0
        const unsigned long long w = __ballot(d);
        pm = d ? c1 : c0;
        wlo = writelane((int)(unsigned)w, tt, wlo);        // lane tt keeps the step's word
        whi = writelane((int)(unsigned)(w >> 32), tt, whi);
    };
    for (int t0 = 0; t0 < T; t0 += 32) {
        const int nt = min(32, T - t0);                    // wave-uniform
        double z = 0.0;
        if (lane < 2 * nt) {
            const int slot = src[2 * (size_t)t0 + lane];
            if (slot >= 0) z = load(slot);                 // a punctured output contributes 0
        }
        const int zlo = __double2loint(z), zhi = __double2hiint(z);
        int wlo = 0, whi = 0;
        if (nt == 32) {
#pragma unroll
            for (int tt = 0; tt < 32; ++tt) step(zlo, zhi, tt, wlo, whi);
        } else {
            for (int tt = 0; tt < nt; ++tt) step(zlo, zhi, tt, wlo, whi);
        }
        if (lane < nt) dec[t0 + lane] = ((unsigned long long)(unsigned)whi << 32) | (unsigned)wlo;
    }
    // the decision words were stored by other lanes of this wave
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

    int s = 0;
    if (!terminated) {                                     // the largest metric, lowest index on ties
        double mx = pm;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) mx = fmax(mx, __shfl_xor(mx, d, 64));
        const unsigned long long eq = __ballot(pm == mx);
        s = eq ? __ffsll((long long)eq) - 1 : 0;
    }
    s = __builtin_amdgcn_readfirstlane(s);
    for (int c0 = ((T - 1) >> 6) << 6; c0 >= 0; c0 -= 64) {
        const int n = min(64, T - c0);
        const unsigned long long w = lane < n ? dec[c0 + lane] : 0ull;
        const int lo = (int)(unsigned)w, hi = (int)(unsigned)(w >> 32);
        unsigned long long bits = 0;
        auto back = [&](int i) {                           // s = the state after step c0 + i
            bits |= (unsigned long long)(s & 1) << i;
            const unsigned wl = (unsigned)__builtin_amdgcn_readlane(lo, i), wh = (unsigned)__builtin_amdgcn_readlane(hi, i);
            const unsigned d = ((s & 32 ? wh : wl) >> (s & 31)) & 1u;
            s = (s >> 1) | (int)(d << 5);
        };
        if (n == 64) {
#pragma unroll
            for (int i = 63; i >= 0; --i) back(i);
        } else {
            for (int i = n - 1; i >= 0; --i) back(i);
        }
        emit(c0, n, bits);
    }
}

// k_viterbi — one wave per codeword of q.cw (CodewordK: placement, lam, counts).
__global__ void __launch_bounds__(256) k_viterbi(CodedK q) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long vit_dec[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long cw = (long long)blockIdx.x * q.wpb + w;
    if (cw >= q.cw.ncw) return;                            // wave-uniform; no block barrier below
    const CodewordAt at = codeword_at(q.cw, cw);
    const int K = q.terminated ? q.T - 6 : q.T;
    int errs = 0;
    viterbi_wave(q.src, q.T, q.terminated, vit_dec + (size_t)w * q.T,
                 [&](int slot) { return codeword_lam(q.cw, at, slot); },
                 [&](int c0, int n, unsigned long long bits) {
                     const int k = K - c0;                  // information bits from step c0 on
                     const unsigned long long mask = k >= 64 ? ~0ull : k <= 0 ? 0ull : (1ull << k) - 1ull;
                     errs += __popcll(bits & mask);
                 });
    if (lane == 0) codeword_count(q.cw, at, errs);
}

void launch_viterbi(hipStream_t s, const CodedK& a) {
    if (a.cw.ncw <= 0) return;
    const long long blocks = (a.cw.ncw + a.wpb - 1) / a.wpb;
    hipLaunchKernelGGL(k_viterbi, dim3((unsigned)blocks), dim3(64 * a.wpb), viterbi_lds(a.T, a.wpb), s, a);
}

// k_viterbi_probe — the same decoder on the caller's lam [ncw][n_slots]; every
// decoded input goes to out [ncw][T], lane i the byte of step c0 + i.
__global__ void __launch_bounds__(256) k_viterbi_probe(const int* __restrict__ src, int T, int terminated, int wpb,
                                                       long long ncw, long long n_slots,
                                                       const double* __restrict__ lam, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long vit_dec[];
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long long cw = (long long)blockIdx.x * wpb + w;
    if (cw >= ncw) return;                                 // wave-uniform
    const double* l = lam + (size_t)cw * (size_t)n_slots;
    uint8_t* o = out + (size_t)cw * (size_t)T;
    viterbi_wave(src, T, terminated, vit_dec + (size_t)w * T, [&](int slot) { return l[slot]; },
                 [&](int c0, int n, unsigned long long bits) {
                     if (lane < n) o[c0 + lane] = (uint8_t)((bits >> lane) & 1ull);
                 });
}

void launch_viterbi_probe(hipStream_t s, const int* src, int T, int terminated, long long ncw, long long n_slots,
                          const double* lam, uint8_t* out) {
    if (ncw <= 0) return;
    const int wpb = viterbi_waves_per_block(T);
    const long long blocks = (ncw + wpb - 1) / wpb;
    hipLaunchKernelGGL(k_viterbi_probe, dim3((unsigned)blocks), dim3(64 * wpb), viterbi_lds(T, wpb), s, src, T, terminated,
                       wpb, ncw, n_slots, lam, out);
}

}  // namespace dsce
