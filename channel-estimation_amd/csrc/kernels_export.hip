// kernels_export.hip — k_export: the way out of the engine for per-realisation
// data (dsce_export, include/dsce.h).  After the receiver front of a batch the
// received grid y [LK][U], the perfect-CSI channel h [LK][R], the pilots xp
// [NP][R] and the transmitted symbol indices sidx [ND][R] sit in the element-
// major buffers of the Monte-Carlo kernels (lane = realisation / unit).  The
// kernel forms the LS pilot estimates (script:412-414, the arithmetic of k_ls)
// and the stage-0 one-tap estimate diag(D_hat) = Wd hP (script:417-428, the
// accumulation order of k_mmse_onetap) from them and writes every requested
// field realisation-major: [rep][snr][element] / [rep][element].  The LS tiles
// run as a launch of their own and also leave the estimates element-major in
// ExportK::hp, from where the h_est tiles of the second launch read them (the
// LS divisions are formed once per unit, not once per h_est tile).
//
// One block = 64 consecutive units (one SNR point, 64 realisations: R is a
// multiple of 64) x one tile of 32 elements of one field.  Phase 1 reads the
// tile with lane = unit (64 x 16 B contiguous per element) into LDS as
// tile[unit][element]; phase 2 reads it back with lane = element and stores 32
// consecutive elements of a realisation per half wave (512 B, 256 B as
// complex64, 128 B of int32).  The row stride of 33 slots is odd, so the 8
// contiguous lanes of a ds_write_b128 group (stride 33 x 16 B) fall into
// distinct 4-bank groups, and a ds_read_b128 lane group reads 16 slots of one
// row at distinct offsets mod 16: both phases are conflict-free.
#include "dsce_kernels.h"

namespace dsce {

static constexpr int XT = EXPORT_TILE;      // elements per tile
static constexpr int XS = XT + 1;           // LDS row stride in slots (odd)

// LS estimate of pilot p for the lane's unit: k_ls's operations in its order
__device__ __forceinline__ double2 export_ls(const ExportK& a, int p, size_t unit, int rl, double sqk) {
    const double2 q = c_div(a.y[(size_t)a.pilot_pos[p] * a.U + unit], a.xp[(size_t)p * a.R + rl]);
    return make_double2(q.x / sqk, q.y / sqk);
}

__device__ __forceinline__ void export_store(void* out, size_t idx, double2 v, bool f32) {
    if (f32) ((float2*)out)[idx] = make_float2((float)v.x, (float)v.y);   // one round-to-nearest per component
    else ((double2*)out)[idx] = v;
}

template <bool F32>
__global__ void __launch_bounds__(256) k_export(ExportK a) {
    __shared__ double2 tile[64 * XS];
    // field and tile of this block: [y | hp_ls | h_est | h | xp | sym]
    int job = blockIdx.y, field = 0;
    while (field < 5 && job >= a.tiles[field]) job -= a.tiles[field++];
    const bool per_unit = field < 3;
    const int first = blockIdx.x * 64;                    // first unit (per-unit fields) / realisation
    if (!per_unit && first >= a.R) return;
    const int snr = per_unit ? a.snr0 + first / a.R : 0;
    const int rl0 = per_unit ? first % a.R : first;
    const int nv = min(64, a.rvalid - rl0);               // realisations of the group that are written
    if (nv <= 0) return;                                  // a wave of tail padding (block-uniform)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int e0 = job * XT;
    const int len = field == 1 || field == 4 ? a.NP : field == 5 ? a.ND : a.LK;
    const int rl = rl0 + lane;
    const size_t unit = (size_t)first + lane;
    const double sqk = 1.0 / a.inv_sqrt_kappa;
    int* itile = (int*)tile;

    if (field == 0 || field == 3 || field == 4) {         // pure moves
        const double2* __restrict__ src = field == 0 ? a.y : field == 3 ? a.h : a.xp;
        const size_t ld = field == 0 ? (size_t)a.U : (size_t)a.R;
        const size_t col = field == 0 ? unit : (size_t)rl;
        for (int e = w; e < XT; e += 4)
            if (e0 + e < len) tile[lane * XS + e] = src[(size_t)(e0 + e) * ld + col];
    } else if (field == 5) {                              // uint16 -> int32
        for (int e = w; e < XT; e += 4)
            if (e0 + e < len) itile[lane * XS + e] = (int)a.sidx[(size_t)(e0 + e) * a.R + rl];
    } else if (field == 1) {                              // LS pilot estimates, kept for the h_est tiles
        for (int e = w; e < XT; e += 4)
            if (e0 + e < len) {
                const double2 v = export_ls(a, e0 + e, unit, rl, sqk);
                a.hp[(size_t)(e0 + e) * a.U + unit] = v;
                tile[lane * XS + e] = v;
            }
        if (!a.out[1]) return;                            // wanted by h_est only (block-uniform)
    } else {                                              // diag(D_hat) = Wd hP, rows e0 + 8 w .. + 7 per wave
        const double2* __restrict__ wd = a.wd + (size_t)snr * a.LK * a.NP;
        double2 acc[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] = make_double2(0.0, 0.0);
#pragma unroll 4
        for (int p = 0; p < a.NP; ++p) {
            const double2 hq = a.hp[(size_t)p * a.U + unit];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = min(e0 + 8 * w + i, a.LK - 1);              // wave-uniform row of Wd
                c_fma(acc[i], wd[(size_t)c * a.NP + p], hq);
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) tile[lane * XS + 8 * w + i] = acc[i];
    }
    __syncthreads();

    // lane = element: 32 consecutive elements of one realisation per half wave
    const int e = threadIdx.x & (XT - 1);
    if (e0 + e >= len) return;
    for (int u = threadIdx.x / XT; u < nv; u += 256 / XT) {
        const long long row = a.row0 + rl0 + u;
        const size_t idx = (size_t)(per_unit ? row * a.nsnr + snr : row) * (size_t)len + (size_t)(e0 + e);
        if (field == 5) ((int*)a.out[5])[idx] = itile[u * XS + e];
        else export_store(a.out[field], idx, tile[u * XS + e], F32);
    }
}

static void launch_tiles(hipStream_t s, const ExportK& a, bool f32) {
    int ntile = 0;
    for (int f = 0; f < 6; ++f) ntile += a.tiles[f];
    if (!ntile) return;
    // per-realisation fields alone need only the R / 64 realisation groups
    const bool units = a.tiles[0] + a.tiles[1] + a.tiles[2] > 0;
    const dim3 grid((units ? a.U : a.R) / 64, ntile);
    if (f32) hipLaunchKernelGGL((k_export<true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_export<false>), grid, dim3(256), 0, s, a);
}

void launch_export(hipStream_t s, const ExportK& a, bool f32) {
    // the LS tiles first (also when only h_est wants them: they fill a.hp), then
    // every other field; the h_est tiles of the second launch read a.hp
    ExportK ls = a, rest = a;
    for (int f = 0; f < 6; ++f) ls.tiles[f] = 0;
    if (a.tiles[1] || a.tiles[2]) ls.tiles[1] = (a.NP + XT - 1) / XT;
    rest.tiles[1] = 0;
    launch_tiles(s, ls, f32);
    launch_tiles(s, rest, f32);
}

// k_export_stages — the stage-aware sibling of k_export (dsce_export_stages): the
// sources are the bulk trace arrays [stage][element][U] that the stage kernels
// filled (TraceK bulk mode), so every field is a pure move.  One block = 64
// consecutive units x one 32-element tile of one (field, stage); the same two
// phases and the same odd-stride LDS tile as k_export.  NaN / -1 entries (formed
// by no kernel of the path) go through as they are.
template <bool F32>
__global__ void __launch_bounds__(256) k_export_stages(ExportStagesK a) {
    __shared__ double2 tile[64 * XS];
    int job = blockIdx.y, field = 0;
    while (field < 4 && job >= a.tiles[field] * a.S) job -= a.tiles[field++] * a.S;
    const int stage = job / a.tiles[field], e0 = (job % a.tiles[field]) * XT;
    const int first = blockIdx.x * 64;                    // first unit of the block (one SNR point: R % 64 == 0)
    const int snr = a.snr0 + first / a.R;
    const int rl0 = first % a.R;
    const int nv = min(64, a.rvalid - rl0);               // realisations of the group that are written
    if (nv <= 0) return;                                  // a wave of tail padding (block-uniform)
    const int lane = threadIdx.x & 63;
    const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int len = a.len[field];
    const bool cplx = field < 3;
    int* itile = (int*)tile;
    const size_t base = (size_t)stage * len;
    if (cplx) {
        const double2* __restrict__ src = (const double2*)a.src[field];
        for (int e = w; e < XT; e += 4)
            if (e0 + e < len) tile[lane * XS + e] = src[(base + e0 + e) * a.U + first + lane];
    } else {
        const int* __restrict__ src = (const int*)a.src[field];
        for (int e = w; e < XT; e += 4)
            if (e0 + e < len) itile[lane * XS + e] = src[(base + e0 + e) * a.U + first + lane];
    }
    __syncthreads();
    // lane = element: 32 consecutive elements of one realisation per half wave
    const int e = threadIdx.x & (XT - 1);
    if (e0 + e >= len) return;
    for (int u = threadIdx.x / XT; u < nv; u += 256 / XT) {
        const long long row = a.row0 + rl0 + u;
        const size_t idx = ((size_t)(row * a.nsnr + snr) * a.S + stage) * (size_t)len + (size_t)(e0 + e);
        if (cplx) export_store(a.out[field], idx, tile[u * XS + e], F32);
        else ((int*)a.out[field])[idx] = itile[u * XS + e];
    }
}

void launch_export_stages(hipStream_t s, const ExportStagesK& a, bool f32) {
    int ntile = 0;
    for (int f = 0; f < 5; ++f) ntile += a.tiles[f] * a.S;
    if (!ntile) return;
    const dim3 grid(a.U / 64, ntile);
    if (f32) hipLaunchKernelGGL((k_export_stages<true>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_export_stages<false>), grid, dim3(256), 0, s, a);
}

}  // namespace dsce
