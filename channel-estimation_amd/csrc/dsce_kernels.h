// dsce_kernels.h — host-callable launchers of the HIP kernels.
#pragma once

#include "dsce_common.h"

#include <vector>

namespace dsce {

// Kernel-selection options of a context (dsce_set_option; defaults = the
// measured-best path).  Read by the launchers; nothing reads the environment.
struct Opts {
    int xcd = 1;              // XCD-aware work order (each XCD walks a contiguous range)
    int fuse_stage = 1;       // MMSE stage of the IC iterations fused into the contraction
    int pic_chain = 3;        // perfect-CSI IC: 0 per-iteration passes, 1 VALU chain, 2 MFMA chain, 3 FFT chain
    int pfuse = 1;            // perfect-CSI detection fused into the second banded pass
    int stage_split = 0;      // 1: 3-kernel stage (k_ls_hest, k_detect, k_precode) for every scheme
    int noise_fuse = 1;       // AWGN drawn inside the Q^H pass (disjoint Q^H blocks)
    int snr_chunk = 0;        // SNR points per receiver chunk (0: all)
    int jakes_rpw = 2;        // realisations per Jakes wave (1 | 2)
    int wtrim = 1;            // trim W to its non-zero column extent (read by dsce_build_mmse)
    int wcontract_valu = 0;   // 1: VALU contraction instead of the MFMA pair tiles
    int mmse_ic = 1;          // MMSE branch of FFT-form OFDM as Q' H_hat G (k_mic_pilot + k_mic_data); 0: W contraction
    int jakes_win = 1;        // Jakes taps only at the samples some Q^H row reads (JakesChunks)
    int txrx_fft = 1;         // TX + channel + receiver front of FFT-form OFDM in one pass (k_txrx_fft)
    int snr_base = 0;         // noise sub-stream of SNR index k is snr_base + k (SNR-sharded sweeps)
    int tx_rows = 1;          // row-local precoders: TX symbols drawn row-parallel (k_tx_rows)
    int realise_win = 0;      // dsce_channel_realise forms only the JakesChunks samples (tests the window kernels)
    int mic_lr = 1;           // MMSE IC taps in the low-rank form T_k Z (k_mic_pilot / k_mic_data) where
                              // build_mic_lr verified it; 0 = the tap GEMM Bv hP on the matrix cores
    int pic_poly = 1;         // perfect-CSI IC passes of polyphase schemes (SchemeK::poly_ok: FBMC, OFDM with
                              // L != 24) as IDFT-L per symbol + window sums per residue + DFT-L per symbol
                              // (k_poly_syn / k_poly_chan / k_poly_ana) instead of the two banded passes
                              // (r04 box, C3: 14.3 -> 8.7 ms per iteration); 0 = the banded passes
    int jakes_grp2 = 1;       // two-tap channels: k_jakes_grp2 (both taps per wave, each Philox block drawn
                              // once, LG = 16 / anchor groups); 0 = k_jakes_grp per tap
    int jakes_mom = 2;        // Jakes taps of the read windows: 2 = Taylor anchors over groups of windows
                              // (k_jakes_grp), 1 = one anchor per window (k_jakes_mom), 0 = recurrence;
                              // each where its truncation is below rounding, else the next lower
    int snr_loop = -1;        // k_pic_fft's SNR-loop form (a block walks the chunk's SNR points of its 64
                              // realisations, the per-realisation prologue once): 1 = wherever it applies,
                              // 0 = never (a block per 64 units), -1 = where the looped grid still fills
                              // the device (launch_perfect_chain)
    int dev_cus = 0;          // not an option: the compute units of the context's device (dsce_create), read
                              // by snr_loop's rule
    int lds_max = 0;          // dynamic LDS in bytes a launch of this context may ask for: the device's
                              // hipDeviceAttributeMaxSharedMemoryPerBlock (dsce_create); dsce_set_option can only
                              // lower it (read by dsce_add_scheme and dsce_build_mmse)
    int export_stage_mb = 1024; // dsce_export_stages: bound in MiB on the bulk trace arrays of one sub-batch
                              // (whole 64-realisation waves; one wave is the floor)
};

// Kernels a scheme's last dsce_run / dsce_trace_unit_ex went through
// (dsce_path_info; bit values mirrored in include/dsce.h DSCE_PATH_*).
enum : unsigned {
    PATH_WPAIR3_FUSED = 1u << 0,   // k_pilot_pre + k_wpair3<.., FUSE> (stage in the contraction epilogue)
    PATH_WPAIR3 = 1u << 1,         // k_wpair3 (3M, unfused)
    PATH_WPAIR4M = 1u << 2,        // retired (r01-r02 k_wpair, 4 real MFMAs per complex product)
    PATH_WCONTRACT_VALU = 1u << 3, // k_wcontract_valu
    PATH_PIC_MFMA = 1u << 4,       // k_pic_mfma (perfect-CSI chain on the matrix cores)
    PATH_PIC_CHAIN = 1u << 5,      // k_pic_chain (VALU chain)
    PATH_PIC_PASSES = 1u << 6,     // G u pass + Q^H H pass per iteration
    PATH_STAGE_FUSED = 1u << 7,    // k_ls + k_stage_fused
    PATH_STAGE_SPLIT = 1u << 8,    // k_ls_hest + k_detect + k_precode
    PATH_NOISE_FUSED = 1u << 9,    // noise drawn inside the Q^H pass
    PATH_PIC_FFT = 1u << 10,       // k_pic_fft (perfect-CSI chain by FFT, OFDM)
    PATH_MIC_FFT = 1u << 11,       // MMSE IC as Q' H_hat G by FFT (OFDM; k_mic_pilot + k_mic_data)
    PATH_TXRX_FFT = 1u << 12,      // k_txrx_fft (TX + channel + noisy receiver front by FFT, OFDM)
    PATH_PILOT_FUSED = 1u << 13,   // retired (r02 k_mic_fft's fused pilot pass)
    PATH_MIC_STAGES = 1u << 14,    // k_mic_pilot + k_mic_data: every MMSE stage in one launch pair
    PATH_MIC_LR = 1u << 15,        // ... with the low-rank tap operator T_k Z (build_mic_lr)
    PATH_PIC_POLY = 1u << 16,      // perfect-CSI IC by polyphase synthesis / analysis (k_poly_*)
    PATH_WROW3 = 1u << 17,         // unfused W contraction as one GEMM per row tile (k_wrow3)
    PATH_SNR_LOOP = 1u << 18,      // k_pic_fft ran in its SNR-loop form (Opts::snr_loop)
};

// Per-stage trace of one unit (dsce_trace_unit_ex): every kernel that forms one
// of these quantities for unit `unit` of the traced scheme writes it here.
// Device arrays, stage-major: [stage][LK] / [stage][ND].
// Bulk mode (U > 0, dsce_export_stages): every unit of the chunk stores, into
// element-major arrays [stage][LK][U] / [stage][ND][U] with the unit fastest, so
// a wave's stores of one element are contiguous.  trace_hit / trace_ix are the
// only readers of unit and U.
struct TraceK {
    int unit;
    int LK, ND;
    double2* yest;     // y_est of stage s (the MMSE IC input y - (D_hat - diag) v), s >= 1
    double2* yperf;    // y_perf of stage s (perfect-CSI IC), s >= 1; null: not wanted (bulk, unless
                       // DSCE_LLR_PERFECT asks for it).  Bulk rows that are formed: the data rows on the
                       // fused select paths (k_pic_fft, StorePerfectDetect: pilot rows and stage 0 stay
                       // NaN), every row of stages >= 1 on the StorePerfectIC path (stage 0 stays NaN)
    double2* hest;     // diag(D_hat) of stage s
    int* dec_e;        // detected symbol index per data symbol, MMSE branch
    int* dec_p;        // perfect-CSI branch
    int U;             // 0: the single unit `unit`; else the chunk's unit count (bulk).  Last, so the
                       // single-unit code of the kernels dsce_run shares with the trace reads the offsets it did
};
// Does `unit` store, and where: e = stage * LK + row (or stage * ND + symbol) is
// the single-unit index, e * U + unit the bulk one.  The <BULK> forms are for
// kernels whose one instance serves dsce_run too (k_stage_fused, k_wpair3): their
// bulk mode is an instance of its own and the other keeps its code.
__device__ __forceinline__ bool trace_hit(const TraceK* t, int unit) { return t->U > 0 || unit == t->unit; }
__device__ __forceinline__ size_t trace_ix(const TraceK* t, size_t e, int unit) {
    return t->U > 0 ? e * (size_t)t->U + (size_t)unit : e;
}
template <bool BULK>
__device__ __forceinline__ bool trace_hit(const TraceK* t, int unit) {
    if constexpr (BULK) return true;
    else return unit == t->unit;
}
template <bool BULK>
__device__ __forceinline__ size_t trace_ix(const TraceK* t, size_t e, int unit) {
    if constexpr (BULK) return e * (size_t)t->U + (size_t)unit;
    else return e;
}

struct McBuffers {
    int R;            // repetitions per batch (multiple of 64)
    int rvalid;       // the first rvalid of them count (a tail batch of a run whose
                      // length is no multiple of 64 pads the last wave; the padding
                      // realisations are simulated but add nothing to any counter)
    int nsnr;
    int U;            // units of the current SNR chunk = nchunk * R, unit = (snr - snr0) * R + rep
    int snr0;         // first SNR index of the chunk being processed
    // per repetition (channel shared by all schemes)
    double2* ir;      // [ntap][N][R]
    // per repetition and scheme
    double2* xp;      // [NP][R]
    uint16_t* sidx;   // [ND][R]
    double2* r0;      // [N][R]
    double2* h;       // [LK][R]   perfect-CSI diag(D)
    double2* xs;      // [LK][R]   scratch: precoded symbols
    double2* ss;      // [N][R]    scratch: time signal
    // per unit
    double2* y;       // [LK][U]
    double2* yest;    // [LK][U]
    double2* yperf;   // [LK][U]
    double2* hp;      // [NP][U]   LS pilot estimates of the current stage
    double2* hp2;     // [NP][U]   second buffer (fused MMSE stage: previous / current stage)
    double2* hest;    // [LK][U]   diag(D_hat) of the current stage
    double2* v;       // [LK][U]   P [xP; Q(x_est)]
    double2* u;       // [LK][U]   P [xP; Q(x_perfect)]
    double2* t;       // [N][U]    scratch: r / G u
    double2* e;       // [LK][U]   y_est ./ h_hat (one-tap quotient, MMSE)
    double2* e2;      // [LK][U]   y_perf ./ h     (one-tap quotient, perfect CSI)
    uint16_t* qe;     // [ND][U]   quantised symbol indices (estimate)
    uint16_t* qp;     // [ND][U]   quantised symbol indices (perfect CSI)
    uint16_t* sidr;   // [LK][R]   transmitted symbol index per data row (row-indexed sidx)
    double2* hpa;     // [stage][NP][U] LS pilot estimates of every stage (k_mic_pilot -> k_mic_data), or null
    int hpa_stages;   // stages hpa holds
    double2* za;      // [stage][ntap * MIC_NB][U] Z = Bz hP of every stage (low-rank MMSE IC), or null
    double2* pv;      // [LK][U] polyphase IC: IDFT of each symbol's C u (k_poly_syn), or null
    double2* pf;      // [LK][U] polyphase IC: window sums of r0 per (symbol, residue), first half (k_poly_chan)
    double2* pf2;     // [LK][U] ... second half; pv / pf / pf2 null unless Opts::pic_poly and a scheme has the form
    double* mse_err;  // null, or [scheme][snr][stage] sums of |h_hat - h|^2 (dsce_enable_mse)
    double* mse_pow;  // [scheme][snr] sums of |h|^2
    const TraceK* tr; // device trace of one unit (null: not tracing this scheme / chunk)
    int tr_bulk;      // tr is in bulk mode (TraceK::U > 0): the launchers pick the bulk instances
    int tr_yperf;     // ... and TraceK::yperf is non-null (DSCE_LLR_PERFECT): the instances that stage y_perf
    bool bulk() const { return tr && tr_bulk; }           // a kernel with a bulk twin launches the twin
    bool bulk_y() const { return bulk() && tr_yperf; }    // ... the twin that stages y_perf
};

struct MmseK {
    const double2* W;     // [var][snr][w_elems] packed band layout
    const double2* Wd;    // [var][snr][LK][NP] diagonal entries W[(c,c),p]
    long long w_elems;
    int nsnr;
    Band Wb;              // block geometry (vals unused; per-(var,snr) base added)
    const double* Wp3;    // [var][snr][3 wp_elems] Re / Im / Re+Im planes (3M form), or null
    long long wp_elems;
    PairBand Pb;
    // fused MMSE stage (block-diagonal W, row-local P): null when not eligible
    const double2* Wpil;  // [var][snr][NP pilots][24 columns][NP]
    const double2* WdA;   // [var][snr][blk][2][NP/4][64] diag(W) rows, MFMA A layout
    const int* pil_c0;    // NP: first column of each pilot row's block
    // structured MMSE IC (k_mic_pilot / k_mic_data): H_hat taps = Bv hP; null when not eligible
    const double2* Bv;    // [var][snr][ntap][N][NP]
    const double2* Bs;    // [var][snr][QH blk][ntap][NP]: Bv summed over each block's FFT window
    const int* pblk;      // QH blocks holding pilot rows (k_pilot_fft)
    int npb;
    const int* dblk;      // QH blocks without pilot rows (k_mic_data)
    int ndb;
    const int* pmask;     // [QH blk]: 1 = holds pilot rows
    // the low-rank form of Bv (build_mic_lr): bv[q][n][p] = sum_k T_k[n] Bz[q k][p],
    // T_k the J0 kernel summed over pilot symbol k's FFT window; null when not eligible
    const double2* Bz;    // [var][snr][ntap * MIC_NB][NP]
    const double* Tw;     // [QH blk][MIC_NB][24]: T_k over the block's FFT window
    const double* Ts;     // [QH blk][MIC_NB]: its window sums
};
// pilot symbols (FFT windows holding pilots) of the low-rank MMSE IC operator
constexpr int MIC_NB = 4;

// Monte-Carlo pipeline.  Launchers return the PATH_* bits of the kernels they ran.
// Chunks of the impulse response a batch needs: every sample some Q^H row of
// some scheme reads (the channel taps are used at output samples only there:
// r0 = H s, diag(D) and the perfect-CSI passes / chains all go through Q^H).
struct JakesChunks {
    static constexpr int LEN = 24;   // samples per chunk
    const int* n0 = nullptr;         // device: first sample of each chunk
    int n = 0;
    std::vector<int> n0h;            // host copy of n0 (the anchor grouping)
    // k_jakes_grp anchor groups (jakes_grouping): runs of consecutive chunks whose
    // span keeps |theta k| <= JAKES_XMAX around the group centre; grp[g] =
    // (first chunk, chunk count); lg lanes per group, mt Taylor terms.  Rebuilt
    // when theta = 2 pi |fD| dt changes; ngrp == 0: not usable.
    const int2* grp = nullptr;
    int ngrp = 0, lg = 0, mt = 0;
    double theta = -1.0;
    int nsch_grp = -1;               // chunk count the groups were built for
};
// the anchor groups' limit: |theta k| <= JAKES_XMAX (the Taylor sum's terms grow
// to e^x / sqrt(2 pi x) before they fall: x = 3 costs ~20x the per-term rounding)
constexpr double JAKES_XMAX = 3.0;
// jc: form only those chunks (samples outside stay as they are: zero).  Returns
// which kernel ran (the work model of dsce_kernel_work): JAKES_KIND_GRP
// k_jakes_grp, JAKES_KIND_MOM k_jakes_mom, else JAKES_KIND_OTHER.
enum { JAKES_KIND_OTHER = 0, JAKES_KIND_MOM = 2, JAKES_KIND_GRP = 3 };
// Which kernel and template instance launch_jakes chose (dsce_jakes_info; the
// kernel values are mirrored in include/dsce.h DSCE_JAKES_*): ngrp / lg / mt
// of the grouped kernels' instance (0 elsewhere), nchunk the window chunks
// formed (0: every sample).
struct JakesInfo {
    int kernel = 0, grp2 = 0, ngrp = 0, lg = 0, mt = 0, nchunk = 0;
};
enum { JAKES_K_NONE = 0, JAKES_K_STATIC = 1, JAKES_K_DISCRETE = 2, JAKES_K_FULL = 3, JAKES_K_WIN_REC = 4,
       JAKES_K_WIN_MOM = 5, JAKES_K_WIN_GRP = 6 };
int launch_jakes(hipStream_t s, const Opts& op, const ChannelK& ch, uint64_t seed, uint64_t rep0, int R,
                  double2* ir, const JakesChunks* jc = nullptr, JakesInfo* info = nullptr);
// txrx (txrx_fft_ok): only the symbols; k_txrx_fft forms s, r0 and diag(D) in
// launch_rx_front
void launch_tx(hipStream_t s, const SchemeK& sk, const ChannelK& ch, int bits_slot, int pilot_slot, uint64_t seed,
               uint64_t rep0, McBuffers& b, bool txrx = false, bool rows = true);
bool txrx_fft_ok(const Opts& op, const SchemeK& sk, const ChannelK& ch, const McBuffers& b);
unsigned launch_rx_front(hipStream_t s, const Opts& op, const SchemeK& sk, const ChannelK& ch, const double* pn,
                         uint64_t seed, uint64_t rep0, McBuffers& b);
unsigned launch_stage(hipStream_t s, const Opts& op, const SchemeK& sk, const MmseK& mm, int stage, int var,
                      int n_iter, bool last, McBuffers& b, unsigned long long* counters, int scheme_index,
                      bool perfect);
// true when launch_stage uses the fused select-mode pass and the precoder is
// row-local, so the perfect-CSI branch of IC iterations can ride on perfect_ic
bool perfect_fusable(const Opts& op, const SchemeK& sk);
unsigned launch_wcontract(hipStream_t s, const Opts& op, const SchemeK& sk, const MmseK& mm, int var, McBuffers& b);
// Fused MMSE stage of IC iteration `stage` (block-diagonal W, row-local P):
// k_pilot_pre (pilot rows + LS into hp_new) then the contraction with the
// stage's detection in its epilogue (no y_est, no separate stage kernel).
bool mmse_fused_ok(const Opts& op, const SchemeK& sk, const MmseK& mm, const McBuffers& b);
void launch_pilot_pre(hipStream_t s, const SchemeK& sk, const MmseK& mm, int var_prev, McBuffers& b,
                      const double2* hp_prev, double2* hp_new);
unsigned launch_mmse_fused(hipStream_t s, const Opts& op, const SchemeK& sk, const MmseK& mm, int var_prev,
                           int var_cur, int stage, int n_iter, bool last, McBuffers& b, const double2* hp_prev,
                           double2* hp_new, unsigned long long* counters, int scheme_index);
// Perfect-CSI detection fused into the perfect IC pass (select mode, row-local P)
struct PerfectDetectArgs {
    unsigned long long* counters;
    int scheme, stage, nstage, nsnr, last;
    double sI, sQ;   // 1 / slicer step (I, Q)
};
// Every MMSE stage (0..n_iter) of an FFT-form OFDM scheme: k_mic_pilot +
// k_mic_data, y_ic = y - Q'(H_hat (G v)) + diag(D_hat) v by the DFT-24 chain;
// the perfect-CSI branch then runs k_pic_fft with its stage 0
bool mmse_stages_ok(const Opts& op, const SchemeK& sk, const MmseK& mm, const ChannelK& ch, const McBuffers& b,
                    int niter);
// part: 1 = k_mic_pilot, 2 = k_mic_data (the data kernel reads the pilot kernel's hpa)
unsigned launch_mmse_stages(hipStream_t s, const SchemeK& sk, const MmseK& mm, const ChannelK& ch, McBuffers& b,
                            const PerfectDetectArgs* pd, int niter, int xcd, int part, bool lr = false);
unsigned launch_perfect_ic(hipStream_t s, const Opts& op, const SchemeK& sk, const ChannelK& ch, McBuffers& b,
                           const PerfectDetectArgs* pd);
// The whole perfect-CSI IC chain (iterations 1..niter) in one kernel, u in
// registers (pic_ok schemes); perfect_chain_ok tells when it applies.
bool perfect_chain_ok(const Opts& op, const SchemeK& sk, const ChannelK& ch, const McBuffers& b, int niter);
// stage0: k_pic_fft also runs the perfect-CSI stage 0 (one-tap y ./ h) first
unsigned launch_perfect_chain(hipStream_t s, const Opts& op, const SchemeK& sk, const ChannelK& ch, McBuffers& b,
                              const PerfectDetectArgs* pd, int niter, bool stage0 = false);
void launch_mmse_onetap(hipStream_t s, int LK, int NP, const double2* wd, const double2* hp, int n, double2* h);

// Bulk export of one batch and SNR chunk after launch_rx_front (k_export,
// kernels_export.hip; dsce_export): LS pilot estimates, the stage-0 one-tap
// estimate Wd hP and the transpose of every requested field from the element-
// major batch buffers to realisation-major outputs.  Fields in the order
// y, hp_ls, h_est, h, xp, sym; tiles[f] = 32-element tiles of field f this
// call writes (0: not requested, or a per-realisation field of a later SNR
// chunk).  Output element of realisation rl (< rvalid; padding realisations are
// written nowhere), SNR index snr: ((row0 + rl) nsnr + snr) len + element for
// the per-unit fields y / hp_ls / h_est, (row0 + rl) len + element for h / xp / sym.
constexpr int EXPORT_TILE = 32;
struct ExportK {
    const double2* y;         // [LK][U]
    const double2* h;         // [LK][R]
    const double2* xp;        // [NP][R]
    const uint16_t* sidx;     // [ND][R]
    const double2* wd;        // [snr][LK][NP]: diag(W) of variant 0 or the interpolation matrix (h_est only)
    double2* hp;              // [NP][U] scratch: the LS estimates, written by the LS tiles, read by the h_est tiles
    const int* pilot_pos;     // NP
    double inv_sqrt_kappa;
    int LK, NP, ND, R, U, snr0, nsnr, rvalid;
    long long row0;           // output row of the batch's realisation 0
    void* out[6];             // device destinations (complex128, or complex64 with f32; sym int32)
    int tiles[6];
};
void launch_export(hipStream_t s, const ExportK& a, bool f32);

// Bulk per-stage export of one batch and SNR chunk after its last stage
// (k_export_stages; dsce_export_stages): the transpose of the bulk trace arrays
// [stage][element][U] to [rep][snr][stage][element].  Fields in the order hp_ls,
// h_est, y_ic (complex), dec_est, dec_perf (int32); tiles[f] = 32-element tiles
// per stage of field f (0: not requested).  Output element of realisation rl
// (< rvalid), SNR index snr, stage s: (((row0 + rl) nsnr + snr) S + s) len + element.
struct ExportStagesK {
    const void* src[5];       // [S][len][U]: double2 (fields 0-2) / int (3, 4); NaN / -1 where nothing was formed
    int len[5];               // NP, LK, LK, ND, ND
    int S, R, U, snr0, nsnr, rvalid;
    long long row0;
    void* out[5];
    int tiles[5];
};
void launch_export_stages(hipStream_t s, const ExportStagesK& a, bool f32);

// Soft demapper of a scheme's constellation (kernels_llr.hip; dsce_llr_awgn,
// dsce_export_llr), derived at dsce_add_scheme.  per_axis: every bit of the label
// depends on one axis of the slicer grid only, so its LLR is a PAM LLR over that
// axis' levels (axis[b]: 0 = I, 1 = Q; mask[b]: the levels where bit b is 1);
// else the full-table form over `symbols` (bit b of symbol i is (i >> b) & 1).
// Passed by value: the tables are kernel arguments (uniform loads).
struct LlrTab {
    const double2* symbols;   // M, sorted by bit label (device)
    int M, m, per_axis;
    int nI, nQ;               // per_axis: levels per axis (<= 16)
    int nbit[2];              // per_axis: bits on each axis
    double lvI[16], lvQ[16];  // ascending, 0 past nI / nQ
    unsigned short mask[8];
    unsigned char axis[8];
};
// Bulk per-stage soft outputs of one batch and SNR chunk after its last stage
// (k_llr; dsce_export_llr): from the bulk trace arrays y_ic / h_est
// [stage][LK][U] the demapper input x_est, its noise power pn_eff and the m LLRs
// of every data symbol, written [rep][snr][stage][ND]( [m]) like k_export_stages.
// Fields in the order x_est (complex), pn_eff, llr (real).  perfect
// (DSCE_LLR_PERFECT): the perfect-CSI branch instead: stage s reads y_perf of
// stage s (y = stage 0 of yic for s = 0) and the channel from h[l][rep]; only the
// rows the demapper needs are read (data_pos, or P^H's columns), see TraceK::yperf.
struct LlrK {
    LlrTab tab;
    const double2* yic;       // [S][LK][U]
    const double2* hest;      // [S][LK][U]
    const double2* yperf;     // [S][LK][U] (stage 0 unused), or null unless perfect
    const double2* h;         // [LK][R] perfect-CSI diag(D) of the batch (perfect, and the pseudo-stage)
    int perfect;              // kernel-uniform: 1 = the perfect-CSI branch at every stage
    const double* pn;         // [nsnr] AWGN power per time sample
    const double* qn;         // [LK] ||Q[:, l]||^2
    const int* data_pos;      // select mode: ND rows
    const int* ph_ptr;        // despread: P^H in CSR (SchemeK::ph_*)
    const int* ph_col;
    const double2* ph_val;
    double data_div;
    int despread, real_detect, maxlog;
    int NP, LK, ND, S, R, U, snr0, nsnr, rvalid;
    long long row0;
    void* out[3];             // null: not requested
    const double* scale;      // [nsnr][S][ND] pn_eff <- scale pn_eff (dsce_set_llr_scale's g_est; perfect:
                              // dsce_set_llr_scale_perf's g_perf), or null
};
void launch_llr(hipStream_t s, const LlrK& a, bool f32);
// BICM information loss of one batch and SNR chunk after its last stage
// (k_llr_info + k_llr_info_sum; dsce_run_soft): k_llr's x_est / pn_eff / LLRs of
// every stage, each LLR turned into loss_b = log2(1 + exp(-(2 t_b - 1) LLR_b))
// with the transmitted bit t_b and summed instead of stored.  k: k_llr's
// arguments (out and row0 unused).  Stage index S is the perfect-CSI one-tap
// receiver: y = stage 0 of yic, the channel from k.h[l][rep] instead of hest.
// With k.perfect the stages 0 .. S - 1 are the perfect-CSI branch's (the pseudo-
// stage is then stage 0 of acc_est and is not asked for).
// One block = 64 units x one tile of LLR_INFO_LT data symbols of one stage; it
// writes its pair of sums (all symbols, considered symbols) to slot
// ((sc nst + st) nb + wave ntile + tile) of `part`, sc the SNR index in the
// chunk, st = stage - st_lo, wave = (unit % R) / 64, nb = (R / 64) ntile.
// k_llr_info_sum then adds each (sc, st)'s nb slots, in slot order, into
// acc_est[snr][stage][2] / acc_perf[snr][2].  No atomics: the sums of two
// identical calls are bit-identical.
constexpr int LLR_INFO_LT = 64;
struct LlrInfoK {
    LlrK k;
    const uint16_t* sidx;     // [ND][R] transmitted symbol indices
    const int* considered;    // ND no-edge flags
    int st_lo, nst;           // stages [st_lo, st_lo + nst) of 0 .. S (S = the perfect-CSI one-tap receiver)
    double* part;             // [chunk SNR points][nst][nb][2] scratch
    double* acc_est;          // [nsnr][S][2], or null
    double* acc_perf;         // [nsnr][2], or null
    const double* scale_perf; // [nsnr][ND] the scale of pseudo-stage S, or null
};
inline size_t llr_info_parts(int ND, int R, int nchunk, int nst) {
    return (size_t)nchunk * nst * (R / 64) * ((ND + LLR_INFO_LT - 1) / LLR_INFO_LT) * 2;
}
void launch_llr_info(hipStream_t s, const LlrInfoK& a);
// Demapper noise ratio of one batch and SNR chunk after its last stage
// (k_llr_calib; dsce_run_calib): k_llr_info's x_est / pn_eff of stages
// [st_lo, st_lo + nst) (stage S = the perfect-CSI one-tap receiver), and per data
// symbol j the sum over the batch's realisations of c |e|^2 / pn_eff, e = x_est -
// symbols[sidx[j][rep]] (real_detect: the real parts, c = 2; else c = 1), added
// into acc_est[snr][stage][j] / acc_perf[snr][j].  k.scale is not read: the ratio
// is against the AWGN pn_eff.  One block = one SNR point of the chunk x one stage
// x one tile of LLR_CALIB_LT symbols; wave w takes the tile's symbols w, w + 4, ..
// and walks the SNR point's unit waves in order, lane = unit, one fp64 sum per
// symbol and lane, then one butterfly per symbol.  Every accumulator entry has
// one writer per launch and a fixed order of terms: no atomics, and the sums of
// two identical calls are bit-identical.
constexpr int LLR_CALIB_LT = 8;
struct LlrCalibK {
    LlrK k;
    const uint16_t* sidx;     // [ND][R] transmitted symbol indices
    int st_lo, nst;
    double* acc_est;          // [nsnr][S][ND], or null
    double* acc_perf;         // [nsnr][ND], or null
};
void launch_llr_calib(hipStream_t s, const LlrCalibK& a);
// What a decoder after k_llr reads about the codewords of one sub-batch and SNR
// chunk (k_viterbi / dsce_run_coded, k_ldpc / dsce_run_ldpc): codeword cw =
// (realisation rl < rvalid, SNR point of the chunk, stage), ncw = rvalid nchunk S
// of them, stage fastest.  llr is k_llr's fp64 output with row0 = 0,
// [R][nsnr][S][B], B = ND m; lam of slot j m + b is that LLR, negated where bit b
// of sidx[j][rl] is 1.  A codeword's decoded ones among its information bits are
// added to acc_bit[snr][stage], and 1 to acc_frame[snr][stage] if there are any,
// with integer atomics: the result does not depend on the order.
struct CodewordK {
    long long ncw;
    const double* llr;        // [R][nsnr][S][B]
    const uint16_t* sidx;     // [ND][R] transmitted symbol indices
    int m, B, S, R, nsnr, snr0, nchunk;
    unsigned long long* acc_bit;     // [nsnr][S], or null
    unsigned long long* acc_frame;   // [nsnr][S], or null
};
// Where codeword cw of a CodewordK lies.  rl is kept widened: as an int the
// compiler extends it again at every load of codeword_lam, which moved k_ldpc's
// iteration loop by 8 bytes and cost 1.5 %.
struct CodewordAt {
    size_t cell;              // snr S + stage: the codeword's entry of the accumulators
    size_t rl;                // its realisation of the sub-batch
    const double* llr;        // its row [B] of llr
};
__device__ __forceinline__ CodewordAt codeword_at(const CodewordK& q, long long cw) {
    const int stage = (int)(cw % q.S);
    const int snr = q.snr0 + (int)((cw / q.S) % q.nchunk);
    const int rl = (int)(cw / ((long long)q.S * q.nchunk));   // < rvalid: padding realisations are not decoded
    CodewordAt at;
    at.cell = (size_t)snr * q.S + stage;
    at.llr = q.llr + (((size_t)rl * q.nsnr + snr) * q.S + stage) * (size_t)q.B;
    at.rl = rl;
    return at;
}
// lam of a slot of the codeword, signed against the transmitted bit
__device__ __forceinline__ double codeword_lam(const CodewordK& q, const CodewordAt& at, int slot) {
    const int j = slot / q.m, b = slot - j * q.m;
    const double v = at.llr[slot];
    const unsigned t = q.sidx[(size_t)j * q.R + at.rl];
    return (t >> b) & 1u ? -v : v;
}
// the codeword's error count into acc_bit / acc_frame; one thread per codeword calls it
__device__ __forceinline__ void codeword_count(const CodewordK& q, const CodewordAt& at, int errs) {
    if (q.acc_bit && errs) atomicAdd(q.acc_bit + at.cell, (unsigned long long)errs);
    if (q.acc_frame && errs) atomicAdd(q.acc_frame + at.cell, 1ull);
}
// K = 7 Viterbi decoder after k_llr (k_viterbi, kernels_viterbi.hip;
// dsce_run_coded): one wave per codeword of cw.  src [T][2] holds slots in
// [-1, B) (checked by the host); the information bits are the first T - 6
// (terminated) or T inputs.  wpb waves per block, each with T decision words of LDS.
struct CodedK {
    const int* src;           // [T][2]
    int T, terminated, wpb;
    CodewordK cw;
};
constexpr int CODE_MAX_STEPS = 8192;  // DSCE_CODE_MAX_STEPS: 8 bytes of decisions per step, 64 KiB per block
inline int viterbi_waves_per_block(int T) { return std::max(1, std::min(4, CODE_MAX_STEPS / std::max(T, 1))); }
inline size_t viterbi_lds(int T, int wpb) { return (size_t)T * wpb * sizeof(unsigned long long); }
void launch_viterbi(hipStream_t s, const CodedK& a);
// the same decoder on lam [ncw][n_slots]: every decoded input to out [ncw][T] (k_viterbi_probe; dsce_viterbi)
void launch_viterbi_probe(hipStream_t s, const int* src, int T, int terminated, long long ncw, long long n_slots,
                          const double* lam, uint8_t* out);
// Normalised min-sum LDPC decoder of include/dsce.h (DSCE_HAS_LDPC_RUN; kernels_ldpc.hip): one workgroup per
// codeword, flooding schedule.  H by check (row_ptr [M + 1], col [E], checked by the host) and by variable (vptr
// [N + 1], vedge [E] = check << 5 | position in the check, a variable's edges in ascending check order); slot [N]
// in [-1, slots).  Dynamic LDS per block: P [N] fp64, then per check m1, m2 (fp64), the sign mask and i1 | sg << 8
// (24 M bytes), then two flag words: ldpc_lds_bytes, compared on the host with Opts::lds_max before any launch.
struct LdpcCodeK {
    const int* row_ptr;       // [M + 1]
    const int* col;           // [E]
    const int* vptr;          // [N + 1]
    const int* vedge;         // [E]
    const int* slot;          // [N]
    int N, M, n_info, max_iter, early_stop;
    double alpha;
};
inline size_t ldpc_lds_bytes(int N, int M) { return (size_t)N * 8 + (size_t)M * 24 + 8; }
// k_ldpc after k_llr (dsce_run_ldpc): one block per codeword of cw, ell = -lam.  The information bits are the first
// n_info variables; the iterations performed go to acc_iter[snr][stage] by an integer atomic as well.
struct LdpcK {
    LdpcCodeK c;
    CodewordK cw;
    unsigned long long* acc_iter;    // [nsnr][S], or null
};
void launch_ldpc(hipStream_t s, const LdpcK& a);
// the same decoder on lam [ncw][n_slots]: x to bits [ncw][N], the iterations performed to iters [ncw] (or null)
// (k_ldpc_probe; dsce_ldpc)
void launch_ldpc_probe(hipStream_t s, const LdpcCodeK& c, long long ncw, long long n_slots, const double* lam,
                       uint8_t* bits, int* iters);
// The layered schedule of the same decoder (DSCE_HAS_LDPC_LAYERED; kernels_ldpc_layered.hip): the lanes of every
// layer, built by the host from H and the checked partition.  Lane i of layer l, lane_ptr[l] <= i < lane_ptr[l + 1],
// is lane[i] = (variable or -1, check << 8 | position << 3 | lg): a check of degree d takes 2^lg >= d consecutive
// lanes (lg 1 .. 5) aligned to 2^lg, positions 0 .. 2^lg - 1, those >= d with variable -1; the groups of a layer
// descend in size, and the layer is filled up to a multiple of 64 lanes with (-1, 31 << 3): lg = 0, never position 0.
// threads = min(1024, the widest layer's lanes).  LdpcCodeK's vptr / vedge are not read.  The same LDS as k_ldpc.
struct LdpcLayersK {
    const int* lane_ptr;      // [n_layers + 1], multiples of 64
    const int2* lane;         // [lane_ptr[n_layers]]
    int n_layers, threads;
};
inline size_t ldpc_layered_lds_bytes(int N, int M) { return ldpc_lds_bytes(N, M); }
struct LdpcLayeredK {
    LdpcCodeK c;
    LdpcLayersK y;
    CodewordK cw;
    unsigned long long* acc_iter;    // [nsnr][S], or null
};
void launch_ldpc_layered(hipStream_t s, const LdpcLayeredK& a);
// (k_ldpc_layered_probe; dsce_ldpc_layered)
void launch_ldpc_layered_probe(hipStream_t s, const LdpcCodeK& c, const LdpcLayersK& y, long long ncw, long long n_slots,
                               const double* lam, uint8_t* bits, int* iters);
// The fixed-point decoder of include/dsce.h (DSCE_HAS_LDPC_FIXED; kernels_ldpc_fixed.hip): LdpcCodeK's tables (alpha
// is not read) and the checked dsce_ldpc_fixed_desc as the integers the kernel uses.  Dynamic LDS per block: two flag
// words, per check an 8-byte record (the two normalised minima as 16 bits each, the sign mask) and i1 | sg << 8 as 16
// bits, then P [N] and ell [N] as int16: ldpc_fixed_lds_bytes, compared on the host with Opts::lds_max.
struct LdpcFixedParK {
    double scale;
    int C, X, A;              // 2^(q - 1) - 1 of the channel, message and a-posteriori words
    int an, sh, half, beta;   // r = max(((mu an + half) >> sh) - beta, 0), half = (1 << sh) >> 1
};
constexpr inline size_t ldpc_fixed_lds_bytes(int N, int M) { return (size_t)N * 4 + (size_t)M * 10 + 8; }
// k_ldpc_fixed after k_llr (dsce_run_ldpc_fixed): one block per codeword of cw; `word` [N] is the caller's codeword
// (0 / 1, checked by the host) or null for the all-zero word.
struct LdpcFixedK {
    LdpcCodeK c;
    LdpcFixedParK f;
    CodewordK cw;
    const uint8_t* word;             // [N], or null
    unsigned long long* acc_iter;    // [nsnr][S], or null
};
void launch_ldpc_fixed(hipStream_t s, const LdpcFixedK& a);
// the same decoder on lam [ncw][n_slots]: x to bits [ncw][N], the iterations performed to iters [ncw] (or null), the
// final P to app [ncw][N] (or null) (k_ldpc_fixed_probe; dsce_ldpc_fixed)
void launch_ldpc_fixed_probe(hipStream_t s, const LdpcCodeK& c, const LdpcFixedParK& f, long long ncw, long long n_slots,
                             const double* lam, uint8_t* bits, int* iters, short* app);
// LLRs of n points x (pn: one value or one per point), out [n][m]
void launch_llr_probe(hipStream_t s, const LlrTab& t, const double2* x, const double* pn, long long n_pn, long long n,
                      bool maxlog, double* out);

// setup (correlation matrices and MMSE estimator)
struct SetupArgs {
    int N, LK, NP, Nsym, ntap, nsnr;
    const int* pilot_pos;
    const double2* G;        // dense N x LK (column-major)
    const double2* Q;        // dense N x LK
    const double2* P;        // dense LK x Nsym
    const double* j0tab;     // 2N-1 time correlation, index lag + N - 1
    int tap_delay[DSCE_MAX_TAPS];
    double pdp[DSCE_MAX_TAPS];
    double kappa;
    const double* pn;        // nsnr
    double thr;
};

void setup_time_correlation(hipStream_t s, int N, double fD, double dt, int model, double* j0tab);
void setup_mcoef(hipStream_t s, const SetupArgs& a, const int* g_start, int GL, const int* q_start, int QL,
                 double2* m /* [NP][ntap][N] */);
void setup_rhp(hipStream_t s, const SetupArgs& a, const double2* m, double2* rhp);
void setup_gp(hipStream_t s, const SetupArgs& a, double2* gp /* N x Nsym */);
void setup_rest_diag(hipStream_t s, const SetupArgs& a, const double2* gp, const int* q_start, int QL, double* diag);
// Dynamic LDS by pilot count, compared on the host with Opts::lds_max before any launch (dsce_add_scheme,
// build_mmse): k_rinv's in-LDS form (used up to RINV_LDS_MAX, the device-memory form beyond), and the [NP][64]
// LS-estimate tile of k_ls_hest and k_wcontract_valu
static constexpr size_t RINV_LDS_MAX = 64 * 1024;
size_t rinv_lds_bytes(int NP);
inline size_t hp_tile_lds_bytes(int NP) { return (size_t)NP * 64 * sizeof(double2); }
void setup_rinv(hipStream_t s, int NP, int nmat, const double2* R, double2* Rinv, double2* work);
// H_hat operator of the structured MMSE IC: bv[sl][q][n][p] = sum_p' m[p'][q][n - d_q]
// Rinv_sl[p'][p] for the nsl = 2 nsnr inverses; bs[sl][blk][q][p] = its sums over
// the FFT windows [klo[blk], klo[blk] + win)
void setup_bv(hipStream_t s, const SetupArgs& a, int nsl, const double2* m, const double2* rinv, double2* bv,
              int nblk, const int* klo, int win, double2* bs);
void setup_rdij(hipStream_t s, const SetupArgs& a, const Band& Wb, const double2* m, const int* g_start, int GL,
                const int* q_start, int QL, double2* rd /* packed, w_elems */);
struct TxDesc {
    int kind, L, K, N, fft, ifb, ts, cp, zg, proto;
    double norm, phase0, rx_scale;
};
// FP64 matrix-core peak microbenchmark: blocks x 4 waves, each `iters` x 8
// independent v_mfma_f64_16x16x4_f64 (2048 flops each)
static constexpr int PEAK_MFMA_PER_ITER = 8;
void launch_mfma_f64_peak(hipStream_t s, int blocks, int iters, double* out);
void setup_tx_matrix(hipStream_t s, const TxDesc& d, const double* proto, double2* G, double2* Q);
// D = Q^H H G of lane `lane` of a Jakes batch `ir` (dsce_transmission_matrix, test probe)
void setup_transmission_matrix(hipStream_t s, const ChannelK& ch, int LK, const double2* ir, int R, int lane,
                               const double2* G, const double2* Q, const int* qlo, const int* qhi, double2* hg,
                               double2* D);
void setup_fused_stage(hipStream_t s, const Band& Wb, int LK, int NP, const double2* w, long long w_elems,
                       const double2* wd, int nslices, const int* pil_blk, const int* pilot_pos, int ncol,
                       double2* wpil, double2* wda);
void setup_wpair(hipStream_t s, const Band& Wb, int NP, const double2* w, long long w_elems, const PairBand& P,
                 double2* wp, long long wp_elems, int nslices, double* w3);
void setup_w_extent(hipStream_t s, const Band& Wb, int NP, const double2* w, long long w_elems, int nslices, int* lohi);
void setup_w(hipStream_t s, const SetupArgs& a, const Band& Wb, long long w_elems, const double2* rd,
             const double2* rinv /* NP x NP */, double2* w /* packed */, double2* wd /* LK x NP */);

}  // namespace dsce
