/*
 * dsce.h — C-ABI of the MI355X doubly-selective channel-estimation engine
 * (libdsce.so).  Plain C types only: pointers + sizes, no torch/HIP types.
 *
 * Reference: rnissel/Channel-Estimation (MATLAB).  The reference has no native
 * layer; these entry points are what a MEX gateway behind the reference's
 * class surfaces binds (see INTEGRATION.md for the gateway and ctypes stubs):
 *
 *   dsce_set_channel      <- Channel.FastFading(...) ctor        FastFading.m:25-192
 *   dsce_channel_realise  <- FastFading.NewRealization +
 *                            .ImpulseResponse / GetConvolutionMatrix
 *                                                               FastFading.m:194-250, :276-295
 *   dsce_add_scheme       <- the operator set of the script     DoublySelectiveChannelEstimation.m:191-205
 *                            (G_*, Q_*, precoders of
 *                             ImaginaryInterferenceCancellationAtPilotPosition.m:37-229,
 *                             PilotMapping_OFDM script:134-142)
 *   dsce_set_snr          <- M_SNR_dB / Pn_time / NrIterations   script:18, :33, :243, :398
 *   dsce_build_mmse       <- correlation matrices + MMSE W      script:208-313 (+ FastFading.m:321-407);
 *                            the 'MMSE' slot of PilotSymbolAidedChannelEstimation
 *                            (stubbed with error() at PSACE.m:110-111)
 *   dsce_run              <- the Monte-Carlo loop body          script:350-564
 *                            ('MMSE' ChannelInterpolation, PSACE.m:128-129, per stage)
 *   dsce_mmse_onetap      <- PilotSymbolAidedChannelEstimation.ChannelInterpolation,
 *                            method 'MMSE' (PSACE.m:128-129 stub): h_hat = diag(sum_p W_p hP_p),
 *                            script:417-428
 *   dsce_get_correlation / dsce_get_W <- R_hP*, W_MMSE_*          script:210-313 (parity probes)
 *   dsce_tx_matrices      <- OFDM/FBMC.GetTXMatrix / GetRXMatrix OFDM.m:184-218, FBMC.m:318-354
 *   dsce_set_interpolation <- PilotSymbolAidedChannelEstimation.ChannelInterpolation,
 *                            'linear'/'nearest'/'FullAverage'/'MovingBlockAverage'
 *                            (PSACE.m:73-107, :115-133) as its LK x NP weight matrix
 *   dsce_set_noise_slot   <- separate n_FBMC / n_OFDM draws     SimpleVersion_DoublyFlat.m:125-126
 *   dsce_export           <- the workspace arrays of the loop body, per realisation:
 *                            y, hP_LS, h_hat (stage 0), h, xP and the data symbols
 *                                                               script:355-368, :388-393, :406-428
 *   dsce_export_stages    <- the same for the IC loop, per realisation and stage:
 *                            hP_LS, h_hat, y after interference cancellation and
 *                            the detected symbols of both CSI branches
 *                                                               script:412-453, :482-548
 *   dsce_llr_awgn         <- SignalConstellation.LLR_AWGN        SignalConstellation.m:103-122
 *   dsce_export_llr       <- the same applied to the demapper input of every stage
 *                            of the MMSE branch                  script:429-444, :519-525
 *   dsce_run_soft         <- no counterpart in the script: the BICM rate of those LLRs
 *                            against the BITS stream, summed per SNR point and stage
 *   dsce_run_calib        <- no counterpart in the script: the demapper error against the
 *                            transmitted symbols over pn_eff, per position
 *   dsce_run_coded        <- no counterpart in the script: the bit and frame errors of a
 *                            K = 7 Viterbi decoder fed with those LLRs, per SNR point and stage
 *   dsce_viterbi          <- the same decoder on the caller's own decoder input
 *   dsce_run_ldpc         <- no counterpart in the script: the bit and frame errors and the
 *                            iterations of a normalised min-sum LDPC decoder on those LLRs
 *   dsce_ldpc             <- the same decoder on the caller's own decoder input
 *   dsce_run_ldpc_layered <- dsce_run_ldpc with the layered schedule over a caller-given
 *                            partition of the checks
 *   dsce_ldpc_layered     <- the layered decoder on the caller's own decoder input
 *   dsce_run_ldpc_fixed   <- dsce_run_ldpc with a fixed-point decoder (word lengths, clip, integer
 *                            normalisation and offset) and a caller-given codeword
 *   dsce_ldpc_fixed       <- the fixed-point decoder on the caller's own decoder input
 *
 * Conventions
 *  - Return 0 on success, a negative DSCE_E* code on failure; the message is
 *    available from dsce_last_error(ctx).  No C++ exception crosses the ABI.
 *  - Complex numbers are interleaved (re, im) doubles; matrices are
 *    column-major like MATLAB (R2018a+ interleaved complex storage).
 *  - Indices are 0-based (a MEX gateway subtracts 1).
 *  - Host buffers are caller-owned and only read/written during the call;
 *    device memory and the HIP stream are owned by the context.
 *  - One context per thread per GPU; no global mutable state besides the HIP
 *    runtime.  A context binds to one HIP device at dsce_create.
 *
 * Random streams (shared with the CPU oracle, oracle/philox.py).
 *  Philox4x32-10 (Salmon et al. 2011), key = (seed & 0xffffffff, seed >> 32),
 *  counter = (idx, rep & 0xffffffff, rep >> 32, stream << 16 | sub).
 *  u53(a,b) = ((a>>5)*2^26 + (b>>6)) * 2^-53.
 *    THETA  (1, 0)   Doppler angles, element e = tap + Ntap*path (MATLAB
 *                    rand([Ntap 1 Paths]) column-major, FastFading.m:227):
 *                    counter e/2, words (0,1) for even e, (2,3) for odd e.
 *    PHI    (2, 0)   random phases, same layout (FastFading.m:233).
 *    BITS   (3, s)   data bits of scheme slot s (script:355-357): bit i is bit
 *                    (i & 31) of word ((i>>5) & 3) of counter i>>7.
 *    PILOTS (4, s)   pilot symbol indices (script:365-367): pilot j is word
 *                    (j & 3) of counter j>>2, masked to log2(M) bits.
 *    NOISE  (5, k + 256 g)  AWGN of SNR index k, shared by all schemes of
 *                    noise slot g (default 0: all schemes, script:399):
 *                    sample e: normal pair of counter e, where a normal pair is
 *                    u1=u53(w0,w1), u2=u53(w2,w3);
 *                    re = sqrt(-2 log(1-u1)) cos(2 pi u2), im = ... sin(2 pi u2).
 *    THETA  (1, 0)   max_doppler == 0: tap q (q-th non-zero tap) is
 *                    1/sqrt(2) sqrt(PDPn) (re + j im) of the normal pair of
 *                    counter q (FastFading.m:244).
 *    THETA  (1, 1)   discrete Doppler models: Doppler bin f = -nd..nd of tap q is
 *                    the normal pair of counter (f + nd) + (2 nd + 1) q
 *                    (GaussUncorr1 / GaussUncorr2, FastFading.m:207-211).
 *
 * Error counters (dsce_run): int64 array of shape
 *   [n_schemes][2 csi: 0 = MMSE estimate, 1 = perfect CSI][2 edge: 0 = all bits,
 *    1 = no-edge bits][n_snr][1 + n_iter stages: 0 = one-tap, i = IC iteration i]
 * (C order, last index fastest).  BER = count / bits, bits from dsce_bits_per_rep.
 *
 * ABI 9 adds dsce_export (dsce_export_out, DSCE_EXPORT_*): per-realisation data
 * in bulk.  Every ABI 8 entry point is unchanged.
 * ABI 10 adds dsce_export_stages (dsce_export_stages_out): the per-stage IC
 * data of every realisation in bulk.  Every ABI 9 entry point is unchanged.
 * DSCE_HAS_LLR (still ABI 10: purely additive) announces dsce_llr_awgn,
 * dsce_export_llr and dsce_llr_info: soft outputs of the demapper.
 * DSCE_HAS_SOFT_RUN (still ABI 10) announces dsce_run_soft: the BICM information
 * loss of those LLRs, summed on the device.
 * DSCE_HAS_LLR_SCALE (still ABI 10) announces dsce_run_calib, dsce_set_llr_scale
 * and dsce_get_llr_scale: the demapper noise measured against the transmitted
 * symbols, and the soft calls' pn_eff scaled by it.
 * DSCE_HAS_LLR_PERFECT (still ABI 10) announces the flag DSCE_LLR_PERFECT of
 * dsce_export_llr, dsce_run_soft and dsce_run_calib (the perfect-CSI branch at
 * every stage) with dsce_set_llr_scale_perf and dsce_get_llr_scale_perf.
 * DSCE_HAS_CODED_RUN (still ABI 10) announces dsce_run_coded and dsce_viterbi:
 * the coded bit and frame errors of a K = 7 Viterbi decoder on the device.
 * DSCE_HAS_LDPC_RUN (still ABI 10) announces dsce_run_ldpc and dsce_ldpc: the
 * same counts from a normalised min-sum decoder of a caller-given LDPC code.
 * DSCE_HAS_LDPC_LAYERED (still ABI 10) announces dsce_run_ldpc_layered and
 * dsce_ldpc_layered: that decoder with the layered schedule.
 * DSCE_HAS_LDPC_FIXED (still ABI 10) announces dsce_run_ldpc_fixed and
 * dsce_ldpc_fixed: the flooding decoder in integers after an input quantiser.
 */
#ifndef DSCE_H
#define DSCE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSCE_ABI_VERSION 10

#define DSCE_OK 0
#define DSCE_EINVAL -1      /* bad argument / shape */
#define DSCE_EHIP -2        /* HIP runtime error */
#define DSCE_ESTATE -3      /* call order (e.g. run before build_mmse) */
#define DSCE_ENOMEM -4

/* How dsce_run sums the members of a context (dsce_group_info) */
#define DSCE_REDUCE_NONE 0  /* a single-device context (dsce_create)                       */
#define DSCE_REDUCE_RCCL 1  /* ncclAllReduce (sum) of the members' device counters, RCCL    */
                            /* over xGMI: dsce_create_multi with distinct devices           */
#define DSCE_REDUCE_HOST 2  /* a device repeats in dsce_create_multi's list (one RCCL rank  */
                            /* per device): the members' counters are summed on the host    */

typedef struct dsce_ctx dsce_ctx;

typedef struct {
    int32_t n_samples;          /* N                                          */
    int32_t n_taps;             /* length of the sampled PDP (incl. zero taps) */
    double sampling_rate;       /* Hz                                         */
    double max_doppler;         /* Hz (FastFading.m:42); 0 = time-invariant    */
                                /* block fading (FastFading.m:241-246)         */
    int32_t n_paths;            /* sum-of-sinusoids paths (FastFading.m:179)   */
    int32_t doppler_model;      /* 0 = 'Jakes', 1 = 'Uniform' (sum of sinusoids, */
                                /* FastFading.m:222-238), 2 = 'Discrete-Jakes', */
                                /* 3 = 'Discrete-Uniform' (IFFT of the discrete */
                                /* Doppler spectrum, FastFading.m:158-177,      */
                                /* :203-221; fD/df <= 0.5 sets fD = 0, :153-156) */
    const double* pdp_norm;     /* n_taps, PowerDelayProfileNormalized (:129) */
} dsce_channel_desc;

/* The frame is caller data.  Accepted: any n_subcarriers, n_symbols >= 1 (LK is
 * no multiple of anything: row blocks may be partial and may straddle symbols),
 * any N (dsce_channel_desc), 1 <= n_pilots <= 64 (no multiple of 4 required),
 * n_data >= 1, n_tx_symbols = n_pilots + n_data, pilot_pos and data_pos anywhere
 * in 0..LK-1 (frame corners and edges included).  Outside that domain
 * dsce_add_scheme returns DSCE_EINVAL ("inconsistent scheme dimensions",
 * "pilot / data position out of range") and adds nothing.  The frame selects
 * kernels, never results: the FFT forms need 24-row blocks on 24-sample windows,
 * the polyphase form L = 24 or 48, the pair-tile contraction NP in {8, 16, 32},
 * the fused stage the same, the structured MMSE IC NP = 16; every other frame
 * runs the banded passes, k_wcontract_valu and k_ls_hest + k_detect + k_precode
 * (tests/geometries.py).
 * LDS: k_ls_hest and k_wcontract_valu keep an [n_pilots][64] complex tile in
 * dynamic LDS (1024 n_pilots bytes: 64 KiB at 64 pilots).  dsce_add_scheme
 * compares that on the host with the context's limit (option lds_max: the
 * device's hipDeviceAttributeMaxSharedMemoryPerBlock unless lowered) and returns
 * DSCE_EINVAL naming n_pilots and the limit when it does not fit, so no launch
 * asks for more than the device gives.  dsce_build_mmse's inverse (k_rinv, 48
 * n_pilots^2 bytes) works in LDS up to 64 KiB (n_pilots <= 36) and in device
 * memory beyond, with the same arithmetic: every n_pilots up to 64 builds. */
typedef struct {
    int32_t n_subcarriers;      /* L >= 1                                      */
    int32_t n_symbols;          /* K >= 1; LK = L*K columns of G and Q         */
    int32_t n_tx_symbols;       /* columns of P: NP + ND                       */
    int32_t n_pilots;           /* NP, 1..64 (DSCE_EINVAL outside)             */
    int32_t n_data;             /* ND >= 1                                     */
    int32_t mod_order;          /* M (power of two, 2..256; larger: DSCE_EINVAL) */
    int32_t bits_per_symbol;    /* log2(M); any of 1..8 (3- and 6-bit symbols   */
                                /* straddle the BITS stream's words, ABI 8)     */
    int32_t despread;           /* 1: x_hat = P^H (y./h), data = entries NP..  (script:436) */
    int32_t real_detect;        /* 1: real() before detection (FBMC-OQAM)      */
    int32_t bits_slot;          /* RNG sub-stream for the data bits            */
    int32_t pilot_slot;         /* RNG sub-stream for the pilots               */
    double kappa;               /* pilot scaling, script:140-142               */
    double data_div;            /* divisor before detection, script:430/437/444 */
    const double* G;            /* N x LK complex, s = G x                     */
    const double* Q;            /* N x LK complex, y = Q^H r                   */
    const double* P;            /* LK x n_tx_symbols complex, x = P [xP; xD]   */
    const int32_t* pilot_pos;   /* n_pilots positions in 0..LK-1               */
    const int32_t* data_pos;    /* n_data positions (select mode)              */
    const uint8_t* considered;  /* n_data no-edge flags (script:151-172)       */
    const double* symbols;      /* M complex, SymbolMapping sorted by bit label. */
                                /* Finite points that fill a rectangular nI x nQ */
                                /* grid (nI nQ = M, any labelling, any offset);  */
                                /* an axis with three or more levels must be     */
                                /* equally spaced: |lv[i] - (lv[0] + i (lv[n-1] -*/
                                /* lv[0]) / (n-1))| <= 1e-9 (lv[n-1] - lv[0]),   */
                                /* the slicers index by (x - lv[0]) / step.      */
                                /* Otherwise DSCE_EINVAL, naming the axis.       */
} dsce_scheme_desc;

/* On-GPU producer of the transmit / receive matrices,
 * replacing Modulation.OFDM/FBMC.GetTXMatrix / GetRXMatrix (OFDM.m:184-218,
 * FBMC.m:318-354): column l + L k of G is the modulated unit impulse of
 * subcarrier l, symbol k, evaluated in closed form per element instead of L
 * Modulation() calls; Q = GetRXMatrix' = G * rx_scale with the OFDM cyclic-
 * prefix samples zeroed (OFDM.m:216-217). */
typedef struct {
    int32_t kind;               /* 0 = OFDM, 1 = FBMC Hermite-OQAM             */
    int32_t n_subcarriers;      /* L                                          */
    int32_t n_symbols;          /* K                                          */
    int32_t n_samples;          /* N = Nr.SamplesTotal                         */
    int32_t fft_size;           /* Implementation.FFTSize                      */
    int32_t intermediate_bin;   /* Implementation.IntermediateFrequency       */
    int32_t time_spacing;       /* Implementation.TimeSpacing (samples)        */
    int32_t cyclic_prefix;      /* OFDM Implementation.CyclicPrefix            */
    int32_t zero_guard;         /* OFDM Implementation.ZeroGuardSamples        */
    int32_t proto_len;          /* FBMC Nr.SamplesPrototypeFilter              */
    double norm;                /* Implementation.NormalizationFactor          */
    double initial_phase;       /* FBMC Implementation.InitialPhaseShift       */
    double rx_scale;            /* GetRXMatrix scale (OFDM L F/SR, FBMC L/(SR T)) */
    const double* prototype;    /* FBMC PrototypeFilter.TimeDomain (proto_len) */
} dsce_tx_desc;

/* Dimensions of a configured scheme, so a binding sizes every output from the
 * engine's own state (dsce_scheme_dims).  n_counters = length of dsce_run's
 * err_counts (all schemes). */
typedef struct {
    int32_t n_samples;          /* N                                          */
    int32_t n_taps;             /* length of the sampled PDP (ImpulseResponse columns) */
    int32_t lk;                 /* L * K                                      */
    int32_t n_pilots;           /* NP                                         */
    int32_t n_data;             /* ND                                         */
    int32_t n_tx_symbols;       /* NP + ND                                    */
    int32_t n_schemes;
    int32_t n_snr;
    int32_t n_iter;
    int64_t n_counters;
} dsce_dims;

/* Per-stage trace of one unit (dsce_trace_unit_ex).  Every pointer is optional
 * (null: not returned).  Complex buffers interleaved; "stage" s = 0 one-tap,
 * s = i IC iteration i; (1 + n_iter) rows, each LK (or NP / ND) long.
 * Entries no kernel of the path forms are NaN (since ABI 4; ABI 3 left 0):
 * e.g. the pilot rows of yperf_stages on the fused perfect-CSI paths, and
 * hest_stages / yest_stages rows of symbols a stage kernel does not visit. */
typedef struct {
    double* y;                  /* LK: y = Q'r                                    script:406-409 */
    double* h_perfect;          /* LK: diag(D), D = Q'HG                           script:388-393 */
    double* hp_stages;          /* (1+n_iter) x NP: LS pilot estimates             script:412-414, :487-489 */
    double* hest_stages;        /* (1+n_iter) x LK: diag(D_hat)                    script:417-428, :493-515 */
    double* yest_stages;        /* (1+n_iter) x LK: y_est = y - (D_hat - diag) v   script:482-484 (row 0 = y) */
    double* yperf_stages;       /* (1+n_iter) x LK: y_perf = y - (D - diag h) u    script:541-543 (row 0 = y;
                                   data rows only on the fused perfect-CSI paths) */
    int32_t* dec_est;           /* (1+n_iter) x ND: detected symbol index, MMSE    script:431, :527 */
    int32_t* dec_perf;          /* (1+n_iter) x ND: detected symbol index, perfect script:453, :548 */
} dsce_trace;

/* Kernel paths (dsce_path_info) */
#define DSCE_PATH_WPAIR3_FUSED    (1u << 0)   /* k_pilot_pre + k_wpair3 with the MMSE stage in its epilogue */
#define DSCE_PATH_WPAIR3          (1u << 1)   /* k_wpair3: MFMA pair-tile contraction, 3M products        */
#define DSCE_PATH_WPAIR4M         (1u << 2)   /* retired in r03 (k_wpair, 4M products); never set          */
#define DSCE_PATH_WCONTRACT_VALU  (1u << 3)   /* k_wcontract_valu                                         */
#define DSCE_PATH_PIC_MFMA        (1u << 4)   /* retired in ABI 4 (k_pic_mfma); never set                  */
#define DSCE_PATH_PIC_CHAIN       (1u << 5)   /* retired in ABI 4 (k_pic_chain); never set                 */
#define DSCE_PATH_PIC_PASSES      (1u << 6)   /* perfect-CSI IC as two banded passes per iteration         */
#define DSCE_PATH_STAGE_FUSED     (1u << 7)   /* k_ls + k_stage_fused                                      */
#define DSCE_PATH_STAGE_SPLIT     (1u << 8)   /* k_ls_hest + k_detect + k_precode                          */
#define DSCE_PATH_NOISE_FUSED     (1u << 9)   /* AWGN drawn inside the Q^H pass                            */
#define DSCE_PATH_PIC_FFT         (1u << 10)  /* k_pic_fft: perfect-CSI IC chain by FFT (OFDM, VALU)       */
#define DSCE_PATH_MIC_FFT         (1u << 11)  /* MMSE IC as Q' H_hat G by FFT (OFDM; with DSCE_PATH_MIC_STAGES) */
#define DSCE_PATH_TXRX_FFT        (1u << 12)  /* k_txrx_fft: TX + channel + noisy receiver front by FFT (OFDM) */
#define DSCE_PATH_PILOT_FUSED     (1u << 13)  /* retired in r03 (k_mic_fft's fused pilot pass); never set     */
#define DSCE_PATH_MIC_STAGES      (1u << 14)  /* k_mic_pilot + k_mic_data: every MMSE stage of an FFT-form OFDM
                                                 scheme in one launch pair; k_pic_fft with the perfect-CSI stage 0 */
#define DSCE_PATH_MIC_LR          (1u << 15)  /* ... with the low-rank tap operator: taps = T_k Z, Z = Bz hP once per
                                                 unit and stage (dsce_structured_check out[5]) */
#define DSCE_PATH_PIC_POLY        (1u << 16)  /* perfect-CSI IC of a polyphase scheme (FBMC; OFDM with L = 48) as
                                                 IDFT-L per symbol + window sums per residue + DFT-L per symbol
                                                 (k_poly_syn / k_poly_chan / k_poly_ana, option pic_poly) */
#define DSCE_PATH_WROW3           (1u << 17)  /* unfused W contraction of 32-row blocks as one GEMM per row tile,
                                                 B = hP v_c (k_wrow3) */
#define DSCE_PATH_SNR_LOOP        (1u << 18)  /* k_pic_fft ran in its SNR-loop form: a block walks the SNR points
                                                 of its 64 realisations (option snr_loop) */

/* Jakes kernels (dsce_jakes_info out6[0]) */
#define DSCE_JAKES_NONE      0   /* no realisation formed yet                                        */
#define DSCE_JAKES_STATIC    1   /* k_static: max_doppler == 0, one value per realisation and tap      */
#define DSCE_JAKES_DISCRETE  2   /* k_discrete: the discrete Doppler models                            */
#define DSCE_JAKES_FULL      3   /* k_jakes, recurrence over every sample (no read windows, option     */
                                 /* jakes_win 0, or more than 256 paths: the windows' LDS tables do    */
                                 /* not fit)                                                           */
#define DSCE_JAKES_WIN_REC   4   /* k_jakes<24, 2, 2>: the recurrence over the read windows            */
#define DSCE_JAKES_WIN_MOM   5   /* k_jakes_mom: one Taylor anchor per window                          */
#define DSCE_JAKES_WIN_GRP   6   /* k_jakes_grp / k_jakes_grp2: Taylor anchors over runs of windows    */

int dsce_abi_version(void);
int dsce_device_count(int* count);

int dsce_create(int hip_device, dsce_ctx** out);
/* Frees the context (every buffer, event and the stream) and returns DSCE_OK,
 * or DSCE_EHIP if a HIP call of the teardown failed (the context is freed
 * either way; the first failing call is named on stderr).  ABI 6: returned
 * void up to ABI 5 (a double free went unseen). */
int dsce_destroy(dsce_ctx* ctx);
const char* dsce_last_error(const dsce_ctx* ctx);

/* Multi-device context (ABI 7; SURVEY §8e, north_star: "realisations shard
 * embarrassingly across the 8 GPUs of one node with a single RCCL all-reduce"),
 * so a host that stays one MATLAB process (README.md:19-20; the loop of
 * DoublySelectiveChannelEstimation.m:350-564) drives every GPU through one
 * handle.  Member i is a context on devices[i] (member 0 is the returned
 * handle).
 *  - Every configuration call — dsce_set_channel, dsce_set_snr,
 *    dsce_add_scheme, dsce_build_mmse (members in parallel: setup is
 *    replicated per device), dsce_set_batch, dsce_set_noise_slot,
 *    dsce_set_interpolation, dsce_set_option, dsce_enable_mse,
 *    dsce_enable_timing — applies to every member (member 0 first; a member's
 *    failure is reported through the handle's dsce_last_error).
 *  - dsce_run splits [first_rep, first_rep + n_rep) into n_devices contiguous
 *    slices on multiples of 64 realisations (dsce/parallel.py shard_range), runs
 *    member i's slice on its own host thread, then sums the members' int64
 *    counters (and MSE sums) with ONE ncclAllReduce per buffer over
 *    communicators from ncclCommInitAll (DSCE_REDUCE_RCCL; devices distinct,
 *    n_devices = 1 included) or on the host when a device repeats
 *    (DSCE_REDUCE_HOST), and adds the total into err_counts once.  The Philox
 *    streams are keyed by the global realisation index, so the counts equal a
 *    single context's bit for bit for any member count.
 *  - Every other call (probes, queries, dsce_kernel_time: member 0's own
 *    launches, i.e. its slice) uses member 0.  dsce_export too: the whole range
 *    is simulated and written by member 0 (DSCE_EXPORT_DEVICE pointers are
 *    memory of devices[0]).
 * dsce_destroy on the handle frees every member and communicator. */
int dsce_create_multi(const int32_t* devices, int32_t n_devices, dsce_ctx** out);
/* Members of a context: *n_devices, their HIP devices (optional, n_devices
 * entries) and *reduce = DSCE_REDUCE_* (each pointer optional). */
int dsce_group_info(dsce_ctx* ctx, int32_t* n_devices, int32_t* devices, int32_t* reduce);

int dsce_set_channel(dsce_ctx* ctx, const dsce_channel_desc* desc);
int dsce_set_snr(dsce_ctx* ctx, const double* pn_time, int32_t n_snr, int32_t n_iter);
int dsce_add_scheme(dsce_ctx* ctx, const dsce_scheme_desc* desc, int32_t* scheme_id);

/* Builds R_hP, R_hP,est, R_hP,est(no interference), R_Dij,hP and the two MMSE
 * estimators W / W0 for every SNR on the GPU, zeroing |.| < zero_threshold
 * like script:263-264, :287-289, :306-308. */
int dsce_build_mmse(dsce_ctx* ctx, double zero_threshold);

/* Repetitions per device batch (default 8192); larger batches fill the GPU
 * better at the cost of HBM for per-unit state. */
int dsce_set_batch(dsce_ctx* ctx, int32_t reps_per_batch);

/* Runs realisations [first_rep, first_rep + n_rep) for every scheme and SNR and
 * ADDS the bit-error counts into err_counts (layout above).  Synchronous.  Any
 * n_rep >= 0 (the script's NrRepetitions = 25 / 1000, script:19 / :44): the
 * device works in whole wavefronts of 64 realisations, and the padding
 * realisations of a tail wave are simulated but counted nowhere (nor in the MSE
 * sums), so counts over [a, b) equal the sum over any split of [a, b). */
int dsce_run(dsce_ctx* ctx, uint64_t seed, uint64_t first_rep, uint64_t n_rep, int64_t* err_counts);

/* Bits per realisation of a scheme: [0] all data bits, [1] no-edge bits. */
int dsce_bits_per_rep(dsce_ctx* ctx, int32_t scheme_id, int64_t* bits2);

/* MMSE one-tap channel for n_units LS pilot-estimate vectors (the 'MMSE' slot of
 * PilotSymbolAidedChannelEstimation): hp_ls is NP x n_units complex
 * (column-major), h_out LK x n_units complex; variant 0 = W, 1 = W0. */
int dsce_mmse_onetap(dsce_ctx* ctx, int32_t scheme_id, int32_t snr_index, int32_t variant, const double* hp_ls,
                     int32_t n_units, double* h_out);

/* G (and Q, each optional) as N x LK complex column-major host buffers. */
int dsce_tx_matrices(dsce_ctx* ctx, const dsce_tx_desc* desc, double* G_out, double* Q_out);

/* Noise slot of a scheme (0..255, default 0): schemes of one slot share the AWGN
 * draw of an SNR point (script:399-403); SimpleVersion_DoublyFlat.m:125-126
 * draws n_FBMC and n_OFDM separately (two slots). */
int dsce_set_noise_slot(dsce_ctx* ctx, int32_t scheme_id, int32_t slot);

/* One-tap channel estimate by a fixed linear interpolation of the LS pilot
 * estimates, h_hat = I hP, instead of the MMSE estimator: the non-'MMSE'
 * methods of PilotSymbolAidedChannelEstimation.ChannelInterpolation
 * (PSACE.m:115-133: 'linear' / 'nearest' scatteredInterpolant weights,
 * 'FullAverage', 'MovingBlockAverage' — all linear in the LS values).
 * I is LK x NP complex, column-major.  The scheme then needs no
 * dsce_build_mmse, and dsce_run requires n_iter == 0 (no W for the IC
 * iterations).  Used by the doubly-flat script, SimpleVersion_DoublyFlat.m:143-145. */
int dsce_set_interpolation(dsce_ctx* ctx, int32_t scheme_id, const double* interp);

/* ---- parity probes (same kernels as dsce_run) ---------------------------- */
/* ImpulseResponse of realisation `rep`: N x n_taps complex, column-major. */
int dsce_channel_realise(dsce_ctx* ctx, uint64_t seed, uint64_t rep, double* ir_out);
/* D = Q^H H G of realisation `rep` for a scheme (script:381-393, the matrix whose
 * diagonal is the perfect-CSI one-tap channel h and whose off-diagonal part the
 * perfect-CSI IC subtracts, script:541-543): LK x LK complex, column-major.  The
 * Monte-Carlo kernels never form D; this probe builds it
 * from the context's dense G / Q and the run's Jakes realisation (ABI 7). */
int dsce_transmission_matrix(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t rep, double* d_out);
/* R_hP (NP x NP), R_est / R_noI (n_snr x NP x NP, each NP x NP column-major). */
int dsce_get_correlation(dsce_ctx* ctx, int32_t scheme_id, double* r_hp, double* r_est, double* r_noi);
/* W (variant 0) or W0 (variant 1) of SNR index k in the reference layout:
 * vector of LK*LK*NP complex, index r + LK*c + LK*LK*p (script:283). */
int dsce_get_W(dsce_ctx* ctx, int32_t scheme_id, int32_t snr_index, int32_t variant, double* w_out);
/* Per-unit trace of one (rep, snr): y (LK), then for stages 0..n_iter the LS
 * pilot estimates (NP each) and the MMSE one-tap channel diag(D_hat) (LK each),
 * and the perfect-CSI diag(D) (LK).  Buffers complex, sized by the caller. */
int dsce_trace_unit(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t rep, int32_t snr_index,
                    double* y, double* hp_stages, double* hest_stages, double* h_perfect);

/* Channel-estimation MSE (build-defined: the reference computes no MSE, so
 * this output is parity-unpinned against MATLAB and checked against the
 * oracle only).  While enabled, every dsce_run adds, per scheme, SNR point and
 * stage (0 = one-tap, i = IC iteration i), the sum over realisations and the
 * LK positions of |h_hat - h|^2, h_hat = diag(D_hat) the stage's MMSE (or
 * interpolation) estimate and h = diag(D) the perfect-CSI one-tap channel of
 * script:450-466; and per scheme and SNR point the sum of |h|^2 (NMSE =
 * err / pow).  err_sum [n_schemes][n_snr][1 + n_iter], pow_sum
 * [n_schemes][n_snr], totals since the last dsce_enable_mse(ctx, 1). */
int dsce_enable_mse(dsce_ctx* ctx, int32_t enable);
int dsce_get_mse(dsce_ctx* ctx, double* err_sum, double* pow_sum);

/* Same kernels as dsce_run (a 64-realisation batch starting at `rep`, the traced
 * unit at its lane 0), with every stage's intermediate quantities of one
 * (rep, snr) unit returned through `out` (see dsce_trace). */
int dsce_trace_unit_ex(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t rep, int32_t snr_index,
                       const dsce_trace* out);

/* ---- bulk export (ABI 9) ------------------------------------------------ */
#define DSCE_EXPORT_F32     (1u << 0)  /* complex64 / float outputs instead of complex128 */
#define DSCE_EXPORT_DEVICE  (1u << 1)  /* every non-null pointer is device memory on the context's GPU */

typedef struct {               /* every pointer optional; realisation-major, C order, element fastest */
    void*    y;        /* [n_rep][n_snr][LK]  y = Q'r                      script:406-409 */
    void*    hp_ls;    /* [n_rep][n_snr][NP]  LS pilot estimates           script:412-414 */
    void*    h_est;    /* [n_rep][n_snr][LK]  diag(D_hat), stage 0: W (variant 0) or the
                          interpolation matrix of dsce_set_interpolation   script:417-428 */
    void*    h;        /* [n_rep][LK]         diag(D), perfect CSI         script:388-393 */
    void*    xp;       /* [n_rep][NP]         unit-modulus pilots          script:365-368 */
    int32_t* sym;      /* [n_rep][ND]         transmitted data symbol index (bi2de of the BITS stream) */
} dsce_export_out;

/* Realisations [first_rep, first_rep + n_rep) of one scheme, every SNR point, as
 * the arrays of dsce_export_out: the Philox streams and the Jakes / TX /
 * receiver-front kernels of dsce_run with the context's options, so realisation
 * `rep` of an export is realisation `rep` of a run with the same seed.  The
 * export stops after the receiver front: no IC stage, no perfect-CSI chain, and
 * nothing is added to the error counters, the MSE sums or dsce_path_info.
 * Works batch by batch (dsce_set_batch) and SNR chunk by SNR chunk (option
 * snr_chunk); the padding realisations of a tail wave are written nowhere.  Any
 * n_rep >= 0.  Synchronous.  Complex outputs are interleaved (re, im) doubles,
 * or floats with DSCE_EXPORT_F32 (each fp64 value rounded once, to nearest, at
 * the store).  Host destinations go through a device staging buffer of one
 * batch; with DSCE_EXPORT_DEVICE the kernel writes the caller's device memory.
 * DSCE_ESTATE before channel, SNR points or scheme are set, and for h_est
 * without a built W (dsce_build_mmse) or an interpolation matrix — the other
 * fields need neither.  DSCE_EINVAL for a null out, no field requested, an
 * unknown flag, or DSCE_EXPORT_DEVICE with a pointer that is not device memory
 * of the context's GPU.  With dsce_enable_timing the kernel is "k_export". */
int dsce_export(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                uint32_t flags, const dsce_export_out* out);

/* ---- bulk per-stage export (ABI 10) -------------------------------------- */
typedef struct {            /* every pointer optional; C order, element fastest; S = 1 + n_iter */
    void*    hp_ls;     /* [n_rep][n_snr][S][NP]  LS pilot estimates of stage s       script:412-414, :487-489 */
    void*    h_est;     /* [n_rep][n_snr][S][LK]  diag(D_hat_s), W / W0 per the i <= NrIter/2 switch
                                                                                     script:417-428, :492-515 */
    void*    y_ic;      /* [n_rep][n_snr][S][LK]  y - (D_hat_(s-1) - diag) v_(s-1); stage 0 = y
                                                                                     script:482-484 */
    int32_t* dec_est;   /* [n_rep][n_snr][S][ND]  detected symbol index, MMSE branch   script:431, :527 */
    int32_t* dec_perf;  /* [n_rep][n_snr][S][ND]  detected symbol index, perfect CSI   script:453, :548 */
} dsce_export_stages_out;

/* Realisations [first_rep, first_rep + n_rep) of one scheme, every SNR point and
 * every stage (one-tap + n_iter IC iterations) of both CSI branches: the Philox
 * streams and the kernels of dsce_run with the context's options, on the kernel
 * path dsce_run takes for the scheme, so realisation `rep` is realisation `rep`
 * of a run and of dsce_export with the same seed.  The stage kernels store every
 * unit into element-major staging arrays ([stage][element][unit], the bulk mode
 * of the per-unit trace), and "k_export_stages" (its name under
 * dsce_enable_timing) transposes them to the layouts above.  An entry that no
 * kernel of the path forms is NaN (-1 for the decisions), as in dsce_trace; on
 * the default OFDM and FBMC paths every entry is formed.  Flags, precision,
 * destinations and pointer validation are those of dsce_export.  Works batch by
 * batch and SNR chunk by SNR chunk; a batch is cut into sub-batches of whole
 * 64-realisation waves so that the staging arrays stay within option
 * export_stage_mb MiB (default 1024; one wave is the floor), and the result does
 * not depend on the cut.  Any n_rep >= 0; padding realisations are written
 * nowhere.  Synchronous.  Nothing is added to the error counters, the MSE sums
 * or dsce_path_info.  DSCE_ESTATE before channel, SNR points or scheme are set,
 * and without dsce_build_mmse (an interpolation scheme with n_iter == 0 needs
 * none).  DSCE_EINVAL for a null out, no field requested, an unknown flag or a
 * bad device pointer.  On a multi-device handle the export is member 0's. */
int dsce_export_stages(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                       uint32_t flags, const dsce_export_stages_out* out);

/* ---- soft outputs (DSCE_HAS_LLR; additive, the ABI version stays 10) ------ */
/* Definitions.
 *  Symbol table: symbols[0..M-1] of the scheme, sorted by bit label; bit b of
 *  symbol index i is (i >> b) & 1 (bi2de, LSB first, as the BITS stream and sym
 *  of dsce_export); m = bits_per_symbol.
 *  Exact LLR (SignalConstellation.LLR_AWGN, its sign: positive means bit 1):
 *    LLR_b(x, pn) = log sum_{i: bit_b(i)=1} exp(-|x - s_i|^2 / pn)
 *                 - log sum_{i: bit_b(i)=0} exp(-|x - s_i|^2 / pn),
 *  evaluated in a max-shifted (log-sum-exp) form: finite and accurate for every
 *  finite x and every pn > 0.  The literal formula underflows to +-Inf or 0/0 far
 *  from the constellation or at small pn (about 8 % of the entries of a default
 *  10 dB / 35 dB export), which the reference patches with +-1e10
 *  (SignalConstellation.m:120-121); the engine returns the true finite value.
 *  NaN inputs give NaN.
 *  Max-log LLR (DSCE_LLR_MAXLOG):
 *    LLR_b = (min_{bit_b=0} |x - s_i|^2 - min_{bit_b=1} |x - s_i|^2) / pn.
 *  Demapper input of the MMSE branch, stage s, data symbol j (what the stage
 *  kernels slice, script:429-444, :519-525), with Pn_l = pn_time[snr] ||Q[:, l]||^2
 *  the AWGN power of y_l:
 *    select schemes (OFDM, FBMC auxiliary; l = data_pos[j]):
 *      x_est_j  = y_ic,s[l] / h_est,s[l] / data_div
 *      pn_eff_j = Pn_l / (|h_est,s[l]|^2 data_div^2)
 *    despread schemes (FBMC coded):
 *      x_est_j  = sum_l conj(P[l, NP+j]) y_ic,s[l] / h_est,s[l] / data_div
 *      pn_eff_j = sum_l |P[l, NP+j]|^2 Pn_l / |h_est,s[l]|^2 / data_div^2
 *  With real_detect x_est is the real part (imaginary part stored as 0); pn_eff
 *  stays the complex power: for a real observation exp(-d^2 / pn) is then the
 *  Gaussian density of variance pn / 2, which is what LLR_AWGN assumes.  Stage 0
 *  uses y_ic = y; h_est follows the W / W0 switch as in dsce_export_stages.
 *  This is the AWGN model of LLR_AWGN: the residual interference and the
 *  correlation of the noise between positions are ignored. */
#define DSCE_HAS_LLR 1
#define DSCE_LLR_MAXLOG (1u << 2)      /* shares the flags word of DSCE_EXPORT_* */

/* SignalConstellation.LLR_AWGN (SignalConstellation.m:103-122) of a scheme's
 * constellation: x n complex (interleaved), pn n_pn = 1 (scalar) or n real,
 * llr_out [n][m] doubles.  Needs only dsce_add_scheme.  flags: 0 |
 * DSCE_LLR_MAXLOG.  The arithmetic is the device function of dsce_export_llr.
 * DSCE_EINVAL for null pointers with n > 0, n < 0, n_pn neither 1 nor n, or an
 * unknown flag; n = 0 does nothing. */
int dsce_llr_awgn(dsce_ctx* ctx, int32_t scheme_id, uint32_t flags, const double* x, const double* pn,
                  int64_t n_pn, int64_t n, double* llr_out);

typedef struct {          /* every pointer optional; C order; S = 1 + n_iter */
    void* x_est;          /* [n_rep][n_snr][S][ND]     complex */
    void* pn_eff;         /* [n_rep][n_snr][S][ND]     real    */
    void* llr;            /* [n_rep][n_snr][S][ND][m]  real    */
} dsce_export_llr_out;

/* The sibling of dsce_export_stages for the soft outputs of the MMSE branch:
 * the same run of the stage kernels (realisation `rep` is realisation `rep` of
 * dsce_run, dsce_export and dsce_export_stages with the same seed), then "k_llr"
 * (its name under dsce_enable_timing) forms x_est, pn_eff and the LLRs as
 * defined above from the staged y_ic and h_est of every stage.  Batches, SNR
 * chunks, the export_stage_mb cut, padding realisations, any n_rep >= 0 and the
 * absence of side effects are those of dsce_export_stages.  flags:
 * DSCE_EXPORT_F32 (x_est complex64, pn_eff and llr float, each fp64 value
 * rounded once at the store), DSCE_EXPORT_DEVICE, DSCE_LLR_MAXLOG.  DSCE_ESTATE
 * before channel, SNR points or scheme are set, and without dsce_build_mmse (an
 * interpolation scheme with n_iter == 0 needs none).  DSCE_EINVAL for a null
 * out, no field requested, an unknown flag or a bad device pointer.  On a
 * multi-device handle the export is member 0's.  With DSCE_LLR_PERFECT the three
 * fields are those of the perfect-CSI branch (DSCE_HAS_LLR_PERFECT below). */
int dsce_export_llr(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                    uint32_t flags, const dsce_export_llr_out* out);

/* Which form the demapper of a scheme takes: out2[0] = 1 the per-axis form
 * (every bit of the label depends on one axis of the constellation grid only:
 * the LLR is a PAM LLR over that axis' levels; every Gray map of the reference),
 * 0 the full-table form over all M symbols; out2[1] = m. */
int dsce_llr_info(dsce_ctx* ctx, int32_t scheme_id, int32_t* out2);

/* ---- BICM rate from the LLRs (DSCE_HAS_SOFT_RUN; additive, ABI 10) -------- */
/* Definitions (x_est, pn_eff, LLR_b exact or max-log, the symbol table and the
 * bit convention are those of the soft-output section above).
 *  t_b(rep, j) = bit b of the transmitted symbol index of data symbol j: the sym
 *  of dsce_export.  The information loss of one bit, in bits,
 *    loss_b = log2(1 + exp(-(2 t_b - 1) LLR_b)),
 *  is evaluated as (max(-z, 0) + log1p(exp(-|z|))) / ln 2, z = (2 t_b - 1) LLR_b:
 *  finite for every finite LLR, NaN for NaN, 1 at LLR = 0, -> 0 for a confident
 *  correct bit, about |LLR| / ln 2 for a confident wrong one.  (The engine sums
 *  the numerators and divides by ln 2 once per block of 64 realisations.)
 *  loss_est[snr][stage][edge]: the sum of loss_b over the realisations of the
 *  call, the data symbols j of the edge class (0 = all, 1 = considered[j]) and the
 *  m bits, with the LLRs of the MMSE branch at that stage: exactly what
 *  dsce_export_llr exports.  [n_snr][1 + n_iter][2] doubles, C order.
 *  loss_perf0[snr][edge]: the same sum for the perfect-CSI one-tap receiver:
 *  x_est and pn_eff formed as for stage 0 with h (diag(D), the h of dsce_export)
 *  in place of h_est.  [n_snr][2] doubles.  The perfect-CSI IC stages: call with
 *  DSCE_LLR_PERFECT (DSCE_HAS_LLR_PERFECT below).
 *  Rate: I = m - loss / (n_rep ND_edge) bits per data symbol, ND_edge m from
 *  dsce_bits_per_rep.  With the exact LLRs this is the estimate of the BICM
 *  mutual information of the demapper output (the achievable rate of
 *  bit-interleaved coded modulation under the AWGN model of LLR_AWGN).  With
 *  DSCE_LLR_MAXLOG it is the rate of the mismatched decoder at LLR scaling 1: a
 *  lower bound on what a decoder can get from those LLRs, and it may be negative.
 *  pn_eff holds the AWGN only: where residual interference dominates (high SNR
 *  before cancellation) the exact LLRs are overconfident too, and their figure is
 *  then likewise a mismatched-decoder rate that can be negative. */
#define DSCE_HAS_SOFT_RUN 1
typedef struct {          /* each optional */
    double* loss_est;     /* [n_snr][1 + n_iter][2] */
    double* loss_perf0;   /* [n_snr][2]             */
} dsce_soft_out;

/* ADDS the sums defined above into the caller's host arrays, as dsce_run adds
 * into err_counts.  The run is dsce_export_llr's (realisation `rep` is
 * realisation `rep` of dsce_run with the same seed; batches, SNR chunks, the
 * export_stage_mb cut, padding realisations that contribute nothing, any
 * n_rep >= 0 with n_rep = 0 adding nothing, no change to the error counters, the
 * MSE sums or dsce_path_info), with "k_llr_info" (its name under
 * dsce_enable_timing) after each SNR chunk: the LLRs are reduced on the device,
 * in a fixed order without atomics, so two identical calls return identical
 * bits; a few doubles reach the host once per call.  flags: 0 | DSCE_LLR_MAXLOG
 * | DSCE_LLR_PERFECT; any other bit (DSCE_EXPORT_F32 and DSCE_EXPORT_DEVICE too) is DSCE_EINVAL, as
 * are a null out and no field requested.  DSCE_ESTATE as for dsce_export_llr.
 * On a multi-device handle the call is member 0's. */
int dsce_run_soft(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                  uint32_t flags, const dsce_soft_out* out);

/* ---- measured demapper noise (DSCE_HAS_LLR_SCALE; additive, ABI 10) ------- */
/* Definitions, for scheme sid, SNR point k, stage s and data symbol j, with
 * S = 1 + n_iter; x_est, pn_eff and the symbol table are those of the soft-output
 * section above, and s_t = symbols[sym[rep][j]] is the transmitted symbol (the
 * sym of dsce_export):
 *    e = x_est - s_t,          c = 1   (complex detection)
 *    e = Re(x_est) - Re(s_t),  c = 2   (real_detect: a real observation has
 *                                       variance pn_eff / 2)
 *    ratio_est[k][s][j] = sum over the call's realisations of c |e|^2 / pn_eff,
 *                         MMSE branch, with the unscaled AWGN pn_eff;
 *    ratio_perf0[k][j]  = the same for the perfect-CSI one-tap receiver (y and h
 *                         of dsce_export, as loss_perf0);
 *    rho = ratio / n_rep.
 *  rho = 1 would mean that the AWGN model of LLR_AWGN holds; rho - 1 is the
 *  residual interference plus estimation error to noise ratio of the position.
 *  The sum is normalised per realisation by pn_eff and not averaged in the x
 *  domain: E[1 / |h|^2] diverges under Rayleigh fading, while the AWGN and the
 *  interference in x_est both scale as 1 / |h_est|^2, so the ratio is what stays
 *  stable.
 *  What rho is not: it is a second-moment match.  The interference is neither
 *  Gaussian nor independent of h, so with exact LLRs and pn_eff <- rho pn_eff the
 *  figure of dsce_run_soft is still the rate of a mismatched decoder, only no
 *  longer an absurd one (at high SNR the unscaled figure is far below zero). */
#define DSCE_HAS_LLR_SCALE 1
typedef struct {            /* each optional */
    double* ratio_est;      /* [n_snr][1 + n_iter][ND] */
    double* ratio_perf0;    /* [n_snr][ND]             */
} dsce_calib_out;

/* ADDS the sums defined above into the caller's host arrays, as dsce_run_soft
 * does.  The run is dsce_run_soft's (the same realisations for the same seed;
 * batches, SNR chunks, the export_stage_mb cut, padding realisations that
 * contribute nothing, any n_rep >= 0 with n_rep = 0 adding nothing, no change to
 * the error counters, the MSE sums or dsce_path_info), with "k_llr_calib" (its
 * name under dsce_enable_timing) after each SNR chunk: summed on the device in
 * a fixed order without atomics, so two identical calls return identical bits.
 * It always measures against the unscaled pn_eff: a call with tables installed
 * returns the bits of a call without.  flags must be 0 or DSCE_LLR_PERFECT: any
 * other bit is DSCE_EINVAL, as are a null out and no field requested.  DSCE_ESTATE as for dsce_run_soft.
 * On a multi-device handle the call is member 0's. */
int dsce_run_calib(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                   uint32_t flags, const dsce_calib_out* out);

/* Installs device-resident scale tables g_est [n_snr][1 + n_iter][ND] and
 * g_perf0 [n_snr][ND] (C order; typically rho) for a scheme; a null argument
 * removes that table.  While g_est is installed dsce_export_llr forms
 * pn_eff <- g_est[k][s][j] pn_eff: the exported pn_eff is the scaled one, the
 * LLRs use it, x_est is unchanged to the bit; dsce_run_soft does the same for
 * loss_est and uses g_perf0 for loss_perf0.  dsce_llr_awgn takes the caller's
 * pn and is untouched.  Every entry must be finite and > 0, else DSCE_EINVAL and
 * the installed tables stay as they were.  Needs dsce_set_snr (DSCE_ESTATE) and
 * the scheme, not dsce_build_mmse; dsce_set_snr drops the tables of every
 * scheme, because their shape is its arguments.  A configuration call: on a
 * multi-device handle it reaches every member. */
int dsce_set_llr_scale(dsce_ctx* ctx, int32_t scheme_id, const double* g_est, const double* g_perf0);
/* set2[0] / set2[1] = 1 where g_est / g_perf0 is installed; the tables are
 * copied out, 1.0 everywhere for one that is not installed.  Every pointer
 * optional.  DSCE_ESTATE before dsce_set_snr. */
int dsce_get_llr_scale(dsce_ctx* ctx, int32_t scheme_id, double* g_est, double* g_perf0, int32_t* set2);

/* ---- the perfect-CSI branch of the soft calls (DSCE_HAS_LLR_PERFECT; additive,
 *      ABI 10) -------------------------------------------------------------- */
/* DSCE_LLR_PERFECT, in the flags word shared with DSCE_EXPORT_* and
 * DSCE_LLR_MAXLOG (bit 3 stays an unknown flag), makes dsce_export_llr,
 * dsce_run_soft and dsce_run_calib work on the perfect-CSI branch, with the same
 * output structs and shapes.  Demapper input of stage s, data symbol j:
 *    y_perf,0 = y;   y_perf,s = y - (D - diag h) u_(s-1) for s >= 1 (script:541-543),
 *    u_(s-1) the re-precoded perfect-CSI decisions of stage s - 1 (the dec_perf of
 *    dsce_export_stages); h = diag(D), the h of dsce_export, at every stage;
 *    select schemes:   x_est_j  = y_perf,s[l] / h[l] / data_div
 *                      pn_eff_j = Pn_l / (|h[l]|^2 data_div^2),  l = data_pos[j]
 *    despread schemes: x_est_j  = sum_l conj(P[l, NP+j]) y_perf,s[l] / h[l] / data_div
 *                      pn_eff_j = sum_l |P[l, NP+j]|^2 Pn_l / |h[l]|^2 / data_div^2
 *  with real_detect handled as for the MMSE branch.  Without a table pn_eff does
 *  not depend on the stage.  The arithmetic is the statement sequence of the MMSE
 *  branch and of the one-tap pseudo-stage: a flagged stage 0 returns the bits of
 *  loss_perf0 / ratio_perf0.
 *  dsce_export_llr: x_est, pn_eff and llr are the perfect-CSI branch's.
 *  dsce_run_soft:   loss_est[snr][stage][edge] receives the perfect-CSI sums; a
 *                   non-null loss_perf0 is DSCE_EINVAL (it is stage 0 of the array).
 *  dsce_run_calib:  ratio_est / ratio_perf0 by the same rule; always against the
 *                   unscaled pn_eff.
 *  A flagged call also stages y_perf of every stage, [stage][LK][unit], which
 *  counts towards the export_stage_mb bound; an unflagged call allocates and
 *  stores what it did.  Rows of the staging that a path does not form are not
 *  read: the paths with the detection fused into the perfect-CSI pass (select
 *  schemes with a row-local precoder: OFDM) form the data rows only, pilot rows
 *  and stage 0 (read from y) stay NaN there; the other paths (FBMC auxiliary
 *  and coded) form every row of the stages >= 1 and leave stage 0 NaN.  On the default OFDM and FBMC
 *  paths every requested output entry is formed.  Batches, SNR chunks,
 *  sub-batches, padding realisations, n_rep = 0, the absence of side effects, the
 *  error codes and "member 0's on a multi-device handle" are those of the
 *  unflagged calls, and without the flag every call returns the bits it returned
 *  before.  Not built: both branches in one call. */
#define DSCE_HAS_LLR_PERFECT 1
#define DSCE_LLR_PERFECT (1u << 4)     /* shares the flags word of DSCE_EXPORT_* and DSCE_LLR_MAXLOG */

/* The scale table of the flagged calls: g_perf [n_snr][1 + n_iter][ND] (C order;
 * typically rho of a flagged dsce_run_calib); null removes it.  While installed,
 * the flagged dsce_export_llr and dsce_run_soft form pn_eff <- g_perf[k][s][j]
 * pn_eff, one multiplication after the unscaled value; x_est keeps its bits.
 * g_est and g_perf0 do not touch the flagged calls and g_perf does not touch the
 * unflagged ones.  Every entry must be finite and > 0, else DSCE_EINVAL and the
 * installed table stays.  Needs dsce_set_snr (DSCE_ESTATE) and the scheme, not
 * dsce_build_mmse; dsce_set_snr drops the table.  A configuration call: on a
 * multi-device handle it reaches every member. */
int dsce_set_llr_scale_perf(dsce_ctx* ctx, int32_t scheme_id, const double* g_perf);
/* set1[0] = 1 where g_perf is installed; the table is copied out, 1.0 everywhere
 * when it is not.  Every pointer optional.  DSCE_ESTATE before dsce_set_snr. */
int dsce_get_llr_scale_perf(dsce_ctx* ctx, int32_t scheme_id, double* g_perf, int32_t* set1);

/* ---- coded BER from a K = 7 Viterbi decoder (DSCE_HAS_CODED_RUN; additive,
 *      ABI 10) -------------------------------------------------------------- */
/* Definitions.
 *  Code: rate 1/2, constraint length 7.  Input u_t, with u_t = 0 for t < 0; the
 *  two outputs of trellis step t are
 *    o0 = u_t ^ u_{t-2} ^ u_{t-3} ^ u_{t-5} ^ u_{t-6}   (133 octal)
 *    o1 = u_t ^ u_{t-1} ^ u_{t-2} ^ u_{t-3} ^ u_{t-6}   (171 octal);
 *  the free distance is 10.
 *  State: s holds u_{t-1} in bit 0 through u_{t-6} in bit 5.  The next state is
 *  ns = ((s << 1) | u_t) & 63; the predecessors of ns are p_b = (ns >> 1) | (b << 5)
 *  for b = 0, 1, with input u_t = ns & 1.
 *  Slots: a realisation offers B = ND m coded-bit slots; slot j m + b is bit b of
 *  data symbol j, the [ND][m] flattening of llr in dsce_export_llr.
 *  Code table: src[T][2] gives, for step t and output k, the slot that carries
 *  it, or -1 for a punctured output, which contributes 0.  Interleaving and
 *  puncturing are nothing but this table; the host builds it (dsce/coding.py
 *  make_code: rates 1/2, 2/3, 3/4 and 5/6 with a random interleaver) and the
 *  engine does not know about rates.
 *  Decoder input:
 *    lam[i]  = t_i ? -LLR_i : LLR_i, t_i the transmitted bit of slot i (bit b of
 *              sym[rep][j], the sym of dsce_export): positive means "the
 *              descrambled bit is 1";
 *    z_{t,k} = src[t][k] < 0 ? 0.0 : lam[src[t][k]].
 *  Why this is exact.  The engine does not encode: it simulates the all-zero
 *  codeword under the scrambler t, the BITS stream, which is uniformly random.
 *  The physical transmission depends only on t = c ^ s, with c the codeword and s
 *  the scrambler.  A maximum-likelihood sequence decoder maximises
 *  sum_i (1 - 2 e_i)(1 - 2 t_i) LLR_i over the codewords e = c_hat ^ c (the code is
 *  linear, so e runs over the code as c_hat does).  So the error pattern e depends
 *  only on lam and is independent of c: the decoded information bits of the
 *  all-zero codeword that are not 0 are the bit errors of any codeword sent with
 *  that scrambler.  "Exact" holds where the maximum-likelihood path is unique.  At
 *  an exact tie of two path metrics the fixed tie rule below favours one path by
 *  its labels (b = 0, the lowest state), not by its metric, and which codeword
 *  that is depends on c; for LLRs of a continuous channel such ties have
 *  negligible probability.  lam is expected to be finite: a NaN loses every
 *  comparison, so a codeword with one decodes as "no error".
 *  Decoder (fp64, exactly this order; dsce/coding.py viterbi_decode is the
 *  bit-identical NumPy twin):
 *   1. pm[0] = 0 and pm[s] = -inf otherwise.
 *   2. Per step and next state ns: c_b = (pm[p_b] + (o0(p_b, u) ? z_{t,0} : 0.0))
 *      + (o1(p_b, u) ? z_{t,1} : 0.0), b = 0, 1, u = ns & 1.
 *   3. The decision is d = (c_1 > c_0): a tie, and -inf against -inf, choose b = 0.
 *   4. pm[ns] = d ? c_1 : c_0.  No renormalisation.
 *   5. Traceback starts from state 0 if `terminated`, else from the state of
 *      largest pm, lowest index on ties.
 *   6. The decoded u_t is bit 0 of the state after step t.
 *  Counts: K = T - 6 information bits if `terminated` (the last six inputs are tail
 *  zeros), else K = T; bit_err = the number of decoded u_t = 1 for t < K;
 *  frame_err = 1 if bit_err is non-zero.  One codeword per realisation, SNR point
 *  and stage; BER = bit_err / (n_rep K), FER = frame_err / n_rep.
 *  Not built: both branches in one call, sharding over a multi-device handle.
 *  Another code: the LDPC section below. */
#define DSCE_HAS_CODED_RUN 1
#define DSCE_CODE_MAX_STEPS 8192   /* the decision words of a codeword (8 bytes per step) stay within 64 KiB of LDS */
typedef struct {
    int32_t n_steps;        /* T: 1 .. DSCE_CODE_MAX_STEPS, at least 7 if terminated */
    int32_t terminated;     /* 1: the last six inputs are tail zeros, traceback from state 0 */
    const int32_t* src;     /* [n_steps][2] slot of output k of step t, or -1 (punctured) */
} dsce_code_desc;

typedef struct {            /* each optional */
    int64_t* bit_err;       /* [n_snr][1 + n_iter] */
    int64_t* frame_err;     /* [n_snr][1 + n_iter] */
} dsce_coded_out;

/* ADDS the counts defined above into the caller's int64 host arrays, as dsce_run
 * adds into err_counts.  The run is dsce_run_soft's with a decoder in place of
 * the sum (the same realisations for the same seed; batches, SNR chunks, the
 * export_stage_mb cut, padding realisations that count nowhere, any n_rep >= 0
 * with n_rep = 0 adding nothing, no change to the error counters, the MSE sums or
 * dsce_path_info): after each SNR chunk "k_llr" writes the fp64 LLRs of the chunk
 * into a device temporary in the layout of dsce_export_llr (its bytes count
 * towards export_stage_mb), so they are the bits dsce_export_llr exports for the
 * same flags, installed scale tables included (g_est, or g_perf with
 * DSCE_LLR_PERFECT); then "k_viterbi" (its name under dsce_enable_timing) decodes
 * one codeword per wavefront, lane = state, and adds its counts to device int64
 * accumulators that live for the call.  Integers: any order of summation gives
 * the same counts, and two identical calls return identical counts.  flags: 0 |
 * DSCE_LLR_MAXLOG | DSCE_LLR_PERFECT; any other bit is DSCE_EINVAL, as are a null
 * code or src, n_steps < 1, terminated with n_steps < 7, n_steps >
 * DSCE_CODE_MAX_STEPS, a src entry outside [-1, ND m), a null out and no field
 * requested.  DSCE_ESTATE as for dsce_run_soft.  On a multi-device handle the
 * call is member 0's. */
int dsce_run_coded(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                   uint32_t flags, const dsce_code_desc* code, const dsce_coded_out* out);

/* The same decoder (the device function of dsce_run_coded, with another load and
 * store) for caller-supplied lam [n_cw][n_slots]: nothing is descrambled, and any
 * codeword is decoded.  info_out [n_cw][n_steps]: all n_steps decoded inputs of
 * every codeword, 0 / 1.  Needs only a context: no scheme, channel or SNR point
 * has to be set.  DSCE_EINVAL for the code errors above (src entries in [-1,
 * n_slots)), n_slots < 0, n_cw < 0 and null data pointers with n_cw > 0; n_cw = 0
 * does nothing. */
int dsce_viterbi(dsce_ctx* ctx, const dsce_code_desc* code, int64_t n_slots, const double* lam, int64_t n_cw,
                 uint8_t* info_out);

/* ---- coded BER from a normalised min-sum LDPC decoder (DSCE_HAS_LDPC_RUN;
 *      additive, ABI 10) ---------------------------------------------------- */
/* Definitions.
 *  Code: any binary parity-check matrix H with M = n_checks rows and N = n_vars
 *  columns, given by check in CSR form: the variables of check c are
 *  col[row_ptr[c] .. row_ptr[c+1] - 1], strictly ascending (no variable twice, and
 *  the position p of a variable in its check is fixed by that order).  A check
 *  joins 2 .. DSCE_LDPC_MAX_CHECK_DEGREE = 32 variables: a check of one variable
 *  would send +-inf and then form inf - inf, and 32 lets the signs of a check be
 *  one 32-bit mask.  A variable may be in any number of checks, none included.
 *  Slots: those of dsce_run_coded, slot j m + b = bit b of data symbol j.  slot[v]
 *  is the slot that carries variable v, or -1 for a punctured or shortened
 *  variable, which contributes 0.0.  Interleaving is nothing but this table, and a
 *  slot may carry more than one variable.  Variables 0 .. n_info - 1 are the
 *  information bits: the host orders the variables so (dsce/coding.py make_ldpc
 *  builds systematic repeat-accumulate codes of rates 1/2, 2/3, 3/4 and 5/6; the
 *  engine does not know about rates or constructions).
 *  Decoder input: lam as for dsce_run_coded, lam[i] = t_i ? -LLR_i : LLR_i,
 *  positive means "the descrambled bit is 1".
 *  Decoder (fp64, exactly this order, no clipping, no renormalisation, no fused
 *  multiply-add; dsce/coding.py ldpc_decode is the bit-identical NumPy twin):
 *   1. ell_v = slot[v] < 0 ? 0.0 : -lam[slot[v]].  Inside the decoder POSITIVE MEANS
 *      "THE BIT IS 0", the opposite of lam: with that convention the sign of a
 *      check's message is the plain XOR of the other signs; with lam's own
 *      convention it would depend on the parity of the check's degree.  The
 *      negation is exact.
 *   2. P_v = ell_v, and R_{c,p} = 0.0 for every edge (p = position in check c).
 *   3. One iteration, flooding schedule (every check reads the P and R of the
 *      previous iteration):
 *      check c with variables v_0 .. v_{d-1}:
 *        q_p = P_{v_p} - R_{c,p},  a_p = |q_p|,  s_p = (q_p < 0);
 *        m1 = min_p a_p, i1 = the lowest p attaining it, m2 = min over p != i1 of
 *        a_p, sg = XOR of all s_p;
 *        mu_p = (p == i1 ? m2 : m1),  r = alpha * mu_p (one rounded product);
 *        R'_{c,p} = (sg ^ s_p) ? -r : r;
 *      variable v, its edges e1, e2, .. in ascending check order:
 *        P'_v = ((ell_v + R'_{e1}) + R'_{e2}) + ...;
 *      x_v = (P'_v < 0);
 *      it += 1; if early_stop is set and every check's XOR of x is 0, stop.
 *   4. After max_iter iterations at the latest the output is x of the last
 *      iteration performed, and it.
 *  A kernel may keep (m1, m2, i1, sg, the mask of s_p) per check instead of R per
 *  edge: R_{c,p} recomputed from that record is the same bits.
 *  Counts: bit_err = the number of x_v = 1 for v < n_info; frame_err = 1 if
 *  bit_err is non-zero; iter_sum = it.  One codeword per realisation, SNR point and
 *  stage; BER = bit_err / (n_rep n_info), FER = frame_err / n_rep, mean iterations
 *  = iter_sum / n_rep.
 *  Why the all-zero codeword is exact.  As for dsce_run_coded nothing is encoded:
 *  the all-zero codeword is simulated under the scrambler t.  Sending codeword c
 *  instead multiplies ell_v by (1 - 2 c_v).  Both updates are sign-symmetric: if
 *  every P_v and R_{c,p} of one iteration is multiplied by (1 - 2 c_v), then |q_p|
 *  is unchanged, s_p becomes s_p ^ c_{v_p} wherever q_p != 0, sg is unchanged since
 *  the c of a check XOR to 0, so R'_{c,p} is multiplied by (1 - 2 c_{v_p}) and P'_v
 *  by (1 - 2 c_v), exactly (negation commutes with rounding).  By induction x
 *  becomes x ^ c, the syndrome of x is unchanged and so is it.  The decided word
 *  XOR the sent word is the all-zero decode, iteration count included.
 *  The caveat: an exactly zero P_v (or q_p) is decided as 0 whatever c_v is, so in
 *  the all-zero simulation it counts as correct although a transmitted 1 there
 *  would have been an error.  That matters only for a punctured variable that
 *  never receives information; for LLRs of a continuous channel it has negligible
 *  probability, like the Viterbi ties above.  lam is expected to be finite.
 *  Kernel: one workgroup per codeword; P (8 N bytes) and the check records (24 M
 *  bytes) live in dynamic LDS, 8 N + 24 M + 8 bytes in all (51 KiB for N = 2560 at
 *  rate 1/2, 30 KiB at rate 5/6).  The calls compare that on the host with the
 *  context's limit (option lds_max) and return DSCE_EINVAL naming the bytes and the
 *  limit when the code does not fit, before anything is launched.
 *  Not built: several small codewords per workgroup, sum-product (a layered
 *  schedule: the section after this one; offset min-sum, in integers: the section
 *  after that), a device-memory fallback for codes beyond the LDS
 *  limit, a MEX command, both branches in one call, sharding over a multi-device
 *  handle. */
#define DSCE_HAS_LDPC_RUN 1
#define DSCE_LDPC_MAX_CHECK_DEGREE 32
#define DSCE_LDPC_MAX_ITER 100
typedef struct {
    int32_t n_vars;         /* N >= 1 */
    int32_t n_checks;       /* M >= 1 */
    const int32_t* row_ptr; /* [n_checks + 1], row_ptr[0] = 0, each check 2 .. 32 entries */
    const int32_t* col;     /* [row_ptr[n_checks]] variables of each check, strictly ascending */
    const int32_t* slot;    /* [n_vars] slot of variable v, or -1 (punctured / shortened) */
    int32_t n_info;         /* 1 .. n_vars: variables 0 .. n_info - 1 are counted */
    int32_t max_iter;       /* 1 .. DSCE_LDPC_MAX_ITER */
    double alpha;           /* finite, 0 < alpha <= 1 */
    int32_t early_stop;     /* 0 | 1: stop once x satisfies every check */
} dsce_ldpc_desc;

typedef struct {            /* each optional */
    int64_t* bit_err;       /* [n_snr][1 + n_iter] */
    int64_t* frame_err;     /* [n_snr][1 + n_iter] */
    int64_t* iter_sum;      /* [n_snr][1 + n_iter] */
} dsce_ldpc_out;

/* dsce_run_coded with the decoder above: ADDS the counts into the caller's int64
 * host arrays.  The same run (realisations, batches, SNR chunks, the
 * export_stage_mb cut with the k_llr temporary counted, padding realisations that
 * count nowhere, n_rep = 0 adding nothing, no change to the error counters, the
 * MSE sums or dsce_path_info), the same "k_llr" temporary holding the bits of
 * dsce_export_llr for the same flags, installed scale tables included; then
 * "k_ldpc" (its name under dsce_enable_timing) decodes one codeword per workgroup
 * and adds its counts to device int64 accumulators with integer atomics: any order
 * gives the same counts.  flags: 0 | DSCE_LLR_MAXLOG | DSCE_LLR_PERFECT.
 * DSCE_EINVAL, with a message naming the offender and nothing written: any other
 * flag bit; a null code, row_ptr, col or slot; n_vars, n_checks, n_info, max_iter,
 * alpha or early_stop outside the bounds above; row_ptr[0] != 0; a check of degree
 * below 2 or above 32 (so a row_ptr that does not increase); a col entry outside
 * [0, n_vars) or not strictly ascending within its check; a slot entry outside
 * [-1, ND m); a code that does not fit lds_max; a null out and no field requested.
 * DSCE_ESTATE as for dsce_run_coded.  On a multi-device handle the call is member
 * 0's. */
int dsce_run_ldpc(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                  uint32_t flags, const dsce_ldpc_desc* code, const dsce_ldpc_out* out);

/* The same decoder (the device function of dsce_run_ldpc, with another load and
 * store) for caller-supplied lam [n_cw][n_slots]: nothing is descrambled, and any
 * codeword is decoded.  bits_out [n_cw][n_vars]: x of every variable, 0 / 1;
 * iters_out [n_cw] (optional): the iterations performed.  Needs only a context.
 * DSCE_EINVAL for the code errors above (slot entries in [-1, n_slots)), n_slots <
 * 0, n_cw < 0 and a null lam or bits_out with n_cw > 0; n_cw = 0 does nothing. */
int dsce_ldpc(dsce_ctx* ctx, const dsce_ldpc_desc* code, int64_t n_slots, const double* lam, int64_t n_cw,
              uint8_t* bits_out, int32_t* iters_out);

/* ---- the same decoder with the layered schedule (DSCE_HAS_LDPC_LAYERED;
 *      additive, ABI 10) ---------------------------------------------------- */
/* Definitions.  Everything not mentioned is the section above: the code, slots,
 * lam, the sign convention "positive ell = the bit is 0", the record (m1, i1, m2,
 * sg, s_p), alpha, fp64 with no clipping, no renormalisation and no fused
 * multiply-add, and the counts.
 *  Layer partition: n_layers layers, the checks of layer l being
 *  layer_check[layer_ptr[l] .. layer_ptr[l+1] - 1].  Every check appears in exactly
 *  one layer, and no two checks of a layer share a variable: the checks of a layer
 *  may then be processed in any order, or all at once, with the same bits, which
 *  is what lets the device take a layer in parallel without atomics and the NumPy
 *  twin (dsce/coding.py ldpc_decode_layered) be bit-identical.  One check per layer
 *  (the serial schedule) is valid for every code; dsce/coding.py make_layers
 *  builds a partition by first fit in check order.  The host checks the partition
 *  in one walk over the edges.
 *  Decoder (exactly this order):
 *   1. ell_v as above; P_v = ell_v, and R_{c,p} = 0.0 for every edge.
 *   2. One iteration runs the layers l = 0 .. n_layers - 1 in order.  For every
 *      check c of layer l with variables v_0 .. v_{d-1}:
 *        q_p = P_{v_p} - R_{c,p},  a_p = |q_p|,  s_p = (q_p < 0);
 *        m1, i1 (the lowest p attaining the minimum), m2, sg, mu_p and r = alpha *
 *        mu_p (one rounded product) exactly as in the flooding schedule;
 *        R'_{c,p} = (sg ^ s_p) ? -r : r;
 *        P_{v_p} = q_p + R'_{c,p} (one rounded sum), and R_{c,.} <- R'_{c,.}.
 *      A check of a later layer reads the P that the earlier layers of the same
 *      iteration have written.  After the last layer x_v = (P_v < 0) and it += 1;
 *      if early_stop is set and every check's XOR of x is 0, stop.
 *   3. After max_iter iterations at the latest the output is x of the last
 *      iteration performed, and it.  A variable in no check keeps P_v = ell_v.
 *  min is exact and "the lowest p among equal minima" is the lexicographic minimum
 *  of (a_p, p), so a kernel may form the record by any reduction tree.
 *  Why the all-zero codeword stays exact.  The check update is the flooding one,
 *  and P <- q + R' commutes with the sign flip (1 - 2 c_v) as the variable sum did:
 *  if every P_v and R_{c,p} before a check is multiplied by (1 - 2 c_v), then q_p is,
 *  |q_p| is unchanged, sg is unchanged since the c of a check XOR to 0, R'_{c,p} is
 *  multiplied by (1 - 2 c_{v_p}) and so is the new P_{v_p}, exactly.  The induction of
 *  the section above carries over check by check, layer by layer: x becomes x ^ c,
 *  the syndrome and the iteration count are unchanged.  The caveat on exact zeros
 *  is the same.
 *  Kernel: one workgroup per codeword, P and the check records in dynamic LDS, the
 *  same 8 N + 24 M + 8 bytes, compared with lds_max in the same way.  Inside a layer
 *  a lane is an edge: a check takes 2, 4, 8, 16 or 32 consecutive lanes of one wave
 *  and its record is formed by a butterfly over them; a barrier separates the
 *  layers, and with early_stop a read-only pass over the checks takes the syndrome
 *  after the last layer.  The workgroup has as many lanes as the widest layer, 1024
 *  at most; a wider layer is walked in strides.
 *  Not built: a fixed-point or offset form of this schedule (the flooding one: the
 *  section below), sum-product, several codewords per workgroup, a device-memory
 *  fallback for codes beyond the LDS limit, a MEX command, both branches in one
 *  call, sharding over a multi-device handle. */
#define DSCE_HAS_LDPC_LAYERED 1
typedef struct {
    int32_t n_layers;             /* 1 .. n_checks */
    const int32_t* layer_ptr;     /* [n_layers + 1], layer_ptr[0] = 0, strictly increasing, last = n_checks */
    const int32_t* layer_check;   /* [n_checks]: the checks of layer l are layer_check[layer_ptr[l] .. layer_ptr[l+1]-1] */
} dsce_ldpc_layers;

/* dsce_run_ldpc with the decoder above: the same run in every respect (flags 0 |
 * DSCE_LLR_MAXLOG | DSCE_LLR_PERFECT, the "k_llr" temporary, batches, SNR chunks,
 * the export_stage_mb cut, padding realisations, n_rep = 0, counts ADDED into the
 * caller's arrays, no change to the error counters, the MSE sums or
 * dsce_path_info, member 0 on a multi-device handle); the decoder's name under
 * dsce_enable_timing is "k_ldpc_layered".  DSCE_EINVAL, with a message naming the
 * offender, nothing written and nothing launched: every refusal of dsce_run_ldpc;
 * a null layers, layer_ptr or layer_check; n_layers outside 1 .. n_checks;
 * layer_ptr[0] != 0, a layer without a check, layer_ptr[n_layers] != n_checks; a
 * layer_check entry outside [0, n_checks); a check that appears twice (named); two
 * checks of one layer that share a variable (the layer, both checks and the
 * variable named). */
int dsce_run_ldpc_layered(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                          uint32_t flags, const dsce_ldpc_desc* code, const dsce_ldpc_layers* layers,
                          const dsce_ldpc_out* out);

/* dsce_ldpc with the decoder above: lam [n_cw][n_slots], bits_out [n_cw][n_vars],
 * iters_out [n_cw] (optional).  Needs only a context.  DSCE_EINVAL as for dsce_ldpc
 * and for the partition errors above; n_cw = 0 does nothing. */
int dsce_ldpc_layered(dsce_ctx* ctx, const dsce_ldpc_desc* code, const dsce_ldpc_layers* layers, int64_t n_slots,
                      const double* lam, int64_t n_cw, uint8_t* bits_out, int32_t* iters_out);

/* ---- the flooding decoder in fixed point (DSCE_HAS_LDPC_FIXED; additive,
 *      ABI 10) -------------------------------------------------------------- */
/* Definitions.  Everything not mentioned is the flooding section's: the code,
 * slots, lam, the sign convention "positive ell = the bit is 0", the record (m1,
 * i1, m2, sg, s_p), max_iter, early_stop and the counts.  dsce_ldpc_desc is used as
 * it is; its alpha must pass the existing check and is not read.
 *  Words: C = 2^(q_ch-1) - 1, X = 2^(q_msg-1) - 1, A = 2^(q_app-1) - 1: symmetric
 *  ranges [-C, C], [-X, X], [-A, A] of the channel values, the messages and the
 *  a-posteriori sums; the most negative code of each word is not used.  scale is
 *  the number of quantiser steps per LLR unit, so the channel clip is C / scale.
 *  Decoder (every step an exact integer operation except step 1;
 *  dsce/coding.py ldpc_decode_fixed is the bit-identical NumPy twin):
 *   1. Quantiser.  For slot[v] >= 0: t = (-lam[slot[v]]) * scale (one rounded fp64
 *      product), mag = min(floor(|t| + 0.5), C) (|t| + 0.5 one rounded fp64 sum),
 *      ell_v = t < 0 ? -mag : mag: round half away from zero, then saturate.  A NaN
 *      lam gives ell_v = 0; +-inf saturates; slot[v] < 0 gives ell_v = 0.  The
 *      quantiser is odd, Q(-x) = -Q(x).  |t| is compared with C before anything is
 *      converted: no NaN and no value outside [0, C] reaches a float-to-int
 *      conversion.
 *   2. P_v = ell_v, and R_{c,p} = 0 for every edge.
 *   3. Check c with variables v_0 .. v_{d-1}:
 *        q_p = clamp(P_{v_p} - R_{c,p}, -X, X),  a_p = |q_p|,  s_p = (q_p < 0);
 *        m1, i1 (the lowest p attaining the minimum), m2, sg and mu_p exactly as in
 *        the flooding section;
 *        r = max(((mu_p * alpha_num + ((1 << alpha_shift) >> 1)) >> alpha_shift)
 *                - beta, 0):
 *        the normalisation alpha_num / 2^alpha_shift rounded half up, then the
 *        offset; with truncation every unit message would become 0;
 *        R'_{c,p} = (sg ^ s_p) ? -r : r.
 *   4. Variable v: P'_v = clamp(ell_v + sum of R'_e over its edges, -A, A), the sum
 *      taken in int32 (its order is irrelevant, and there is one clamp);
 *      x_v = (P'_v < 0).
 *   5. it, the early stop and the output "x of the last iteration performed" are
 *      the flooding section's.
 *  With integer-valued lam, scale 1, alpha 1 / 1, beta 0 and words wide enough that
 *  nothing clamps, this is the flooding decoder at alpha = 1.0, bit for bit.
 *  Codeword (the run only).  The engine still does not encode: `codeword` [n_vars]
 *  is a word of the code that the caller supplies (dsce/coding.py ldpc_encode
 *  makes one), entries 0 / 1, every check XORing to 0; the host checks both.  The
 *  run is exactly the transmission of c under the scrambler t ^ c, t being the
 *  BITS stream: with ell0_v the value of step 1 from lam signed against t, the
 *  decoder starts from ell_v = c_v ? -ell0_v : ell0_v, runs its plain zero and tie
 *  rules, and bit_err counts x_v ^ c_v for v < n_info; frame_err and iter_sum as
 *  before.  A null codeword is the all-zero word.  That run is OPTIMISTIC: the
 *  sign-symmetry argument of the flooding section holds except where a q_p or a
 *  P_v is exactly 0, which is decided as "bit 0" whatever c_v is; in fp64 such
 *  zeros have negligible probability, in integers zeros and ties are everywhere,
 *  and every one of them is decided in favour of the all-zero word.  Measured on
 *  make_ldpc(2560, "1/2"), BPSK / AWGN at sigma = 0.80, 60 frames, the same noise
 *  (tests/test_ldpc_fixed_host.py): at 3 / 3 / 5 bit, scale 1, unnormalised, the
 *  all-zero word shows 350 wrong information bits and 1514 iterations where real
 *  codewords show 514 and 1615.  On the default OFDM link (8192 realisations,
 *  stage 4, 25 dB, rate 1/2) the FER of the all-zero word is
 *  0.3455 against 0.3671 at 4 / 4 / 6 bit and 0.1353 against 0.1355 at 6 / 6 / 8.
 *  The probe has no codeword: it decodes the caller's lam as it is.
 *  The struct below is dsce_ldpc_fixed_desc because dsce_ldpc_fixed is the probe's
 *  entry point: in C a typedef and a function cannot share a name.
 *  Kernel: one workgroup per codeword; dynamic LDS holds two flag words, an 8-byte
 *  record and a 16-bit i1 | sg per check, and P and ell as int16:
 *  DSCE_LDPC_FIXED_LDS_BYTES(N, M) = 4 N + 10 M + 8 bytes (23 KiB for N = 2560 at
 *  rate 1/2), less than half of the fp64 kernel's, compared with lds_max on the
 *  host in the same way.  No floating point after the quantiser, plain vector
 *  loads and stores, integer atomics for the three counts only.
 *  Not built: a layered fixed-point decoder, sum-product, several codewords per
 *  workgroup, a MEX command, both branches in one call, sharding over a
 *  multi-device handle. */
#define DSCE_HAS_LDPC_FIXED 1
#define DSCE_LDPC_FIXED_LDS_BYTES(N, M) (4 * (int64_t)(N) + 10 * (int64_t)(M) + 8)
typedef struct {
    double  scale;        /* finite, > 0: quantiser steps per LLR unit            */
    int32_t q_ch;         /* 2..16: channel word, C = 2^(q_ch-1) - 1               */
    int32_t q_msg;        /* 2..16: message word,  X = 2^(q_msg-1) - 1              */
    int32_t q_app;        /* max(q_ch, q_msg)..16: a-posteriori word, A = 2^(q_app-1) - 1 */
    int32_t alpha_num;    /* 1 .. 1 << alpha_shift                                 */
    int32_t alpha_shift;  /* 0..8                                                  */
    int32_t beta;         /* 0..32767: offset                                      */
} dsce_ldpc_fixed_desc;

/* dsce_run_ldpc with the decoder above: the same run in every respect (flags 0 |
 * DSCE_LLR_MAXLOG | DSCE_LLR_PERFECT, the "k_llr" temporary, batches, SNR chunks,
 * the export_stage_mb cut, padding realisations, n_rep = 0, counts ADDED into the
 * caller's arrays, no change to the error counters, the MSE sums or
 * dsce_path_info, member 0 on a multi-device handle); the decoder's name under
 * dsce_enable_timing is "k_ldpc_fixed".  codeword [n_vars] or null: see above.
 * DSCE_EINVAL, with a message naming the offender, nothing written and nothing
 * launched: every refusal of dsce_run_ldpc, the LDS need being
 * DSCE_LDPC_FIXED_LDS_BYTES; a null fx; a field of fx outside its bounds; a
 * codeword entry above 1; a codeword that leaves a check unsatisfied (the first
 * such check named). */
int dsce_run_ldpc_fixed(dsce_ctx* ctx, int32_t scheme_id, uint64_t seed, uint64_t first_rep, uint64_t n_rep,
                        uint32_t flags, const dsce_ldpc_desc* code, const dsce_ldpc_fixed_desc* fx,
                        const uint8_t* codeword, const dsce_ldpc_out* out);

/* dsce_ldpc with the decoder above ("k_ldpc_fixed_probe"): lam [n_cw][n_slots],
 * bits_out [n_cw][n_vars], iters_out [n_cw] (optional), app_out [n_cw][n_vars]
 * (optional): the P_v of the last iteration performed.  Needs only a context.
 * DSCE_EINVAL as for dsce_ldpc and for fx as above; n_cw = 0 does nothing. */
int dsce_ldpc_fixed(dsce_ctx* ctx, const dsce_ldpc_desc* code, const dsce_ldpc_fixed_desc* fx, int64_t n_slots,
                    const double* lam, int64_t n_cw, uint8_t* bits_out, int32_t* iters_out, int16_t* app_out);

/* ---- engine state ------------------------------------------------------- */
int dsce_scheme_dims(dsce_ctx* ctx, int32_t scheme_id, dsce_dims* dims);
/* Which kernels a scheme's last dsce_run / trace used: DSCE_PATH_* bits. */
int dsce_path_info(dsce_ctx* ctx, int32_t scheme_id, uint32_t* flags);
/* Which Jakes kernel and template instance formed the channel taps of the last
 * dsce_run batch / trace or dsce_channel_realise (ABI 8; read-only):
 * out6[0] = DSCE_JAKES_*; and for DSCE_JAKES_WIN_GRP out6[1] = 1 for
 * k_jakes_grp2<mt, lg> (both taps of a two-tap channel per wave, lg = 16 /
 * groups), 0 for k_jakes_grp<mt, lg>, out6[2] = anchor groups, out6[3] = lg
 * lanes per anchor (4 | 8 | 16), out6[4] = mt Taylor terms (16 | 24 | 28)
 * (all 0 for the other kernels); out6[5] = the 24-sample window chunks formed
 * (0: every sample). */
int dsce_jakes_info(dsce_ctx* ctx, int32_t* out6);
/* Kernel-selection options (defaults = the measured-best path; each other value
 * selects a real fallback, reached by the parity tests):
 *   xcd (XCD-aware work order), fuse_stage (MMSE stage in the contraction's
 *   epilogue), pic_chain (3: perfect-CSI IC chain by FFT where the scheme's G / Q
 *   allow it, 0: two banded passes per iteration), pfuse, stage_split,
 *   noise_fuse, snr_chunk (0 all), jakes_rpw (1|2), wtrim (read by
 *   dsce_build_mmse), wcontract_valu (the VALU contraction, also the fallback
 *   without pair tiles), mmse_ic (1: the MMSE branch of an FFT-form OFDM scheme
 *   as y - Q'(H_hat (G v)) + diag(D_hat) v with H_hat = E{H | hP}, every stage in
 *   k_mic_pilot + k_mic_data and the perfect-CSI stage 0 in k_pic_fft; equal to
 *   the W contraction of script:482-511 to rounding, checked at dsce_build_mmse;
 *   0: the W contraction everywhere), jakes_win, txrx_fft, jakes_mom (the Jakes
 *   taps of the read windows: 2 = Taylor anchors over runs of windows, 1 = one
 *   anchor per window, 0 = the recurrence; each only where its truncation stays
 *   below rounding), realise_win (1: dsce_channel_realise forms only the samples
 *   the schemes' windows read, zero elsewhere, with the run's Jakes kernels),
 *   tx_rows (1: TX symbols of a row-local precoder drawn row-parallel), snr_base
 *   (0..255: the noise of SNR index k is sub-stream snr_base + k, so a rank
 *   serving SNR points [b, ...) of a sweep draws the one-rank run's noise),
 *   mic_lr (1: the MMSE IC's estimated taps in the low-rank form T_k Z where the
 *   fit reproduces Bv to rounding, dsce_structured_check; 0: the tap GEMM Bv hP),
 *   pic_poly (1: the perfect-CSI IC passes of a scheme whose G and Q factorise as real windows x
 *   subcarrier tones, G[n, l + L k] = A_k[n] e^(2 pi i l n / L) C[l][k], checked
 *   entry by entry to 1e-12 at dsce_add_scheme, with L = 24 or 48, as an IDFT-L
 *   per symbol, window sums per residue n mod L around the channel, and a DFT-L
 *   per symbol, DSCE_PATH_PIC_POLY, the default; 0: the two banded passes),
 *   jakes_grp2 (1, the
 *   default: a channel with two non-zero taps forms the Jakes taps of the read
 *   windows with k_jakes_grp2 — both taps per wave, each Philox block drawn
 *   once; 0: k_jakes_grp, one tap per block; r06), snr_loop (k_pic_fft with its
 *   stage 0: 1 = a block per 64 realisations and symbol walks the chunk's SNR
 *   points, the per-realisation prologue once, DSCE_PATH_SNR_LOOP; 0 = a block
 *   per 64 units; -1, the default: the loop where its grid still fills the
 *   device; same counts either way), lds_max (bytes of dynamic LDS a launch of
 *   the context may ask for; default and ceiling: the device's
 *   hipDeviceAttributeMaxSharedMemoryPerBlock, floor 1024; read by
 *   dsce_add_scheme and dsce_build_mmse, see dsce_scheme_desc, and by
 *   dsce_run_ldpc and dsce_ldpc).
 * Retired after r06 (no scheme or channel selected their other values;
 * DSCE_EINVAL): pic_net, mic_net (the DPP form of the chain kernels' 4-point
 * network; the matrix-core form is the only one), stage_rb (k_stage_fused runs 8
 * rows per wave), wrow (32-row blocks always take k_wrow3, DSCE_PATH_WROW3).
 * Retired in r06 (measured neutral in r04 / r05; DSCE_EINVAL): pic_skip (the
 * perfect-CSI fixed-point exit), ic_streams (the chain on a second stream /
 * beside the pilot pass in one launch, k_ic_pair).
 * Retired in r03 (the r01-r02 variants they selected are gone; DSCE_EINVAL):
 * wpair_3m, wda_3m, streams, qidx, stage0_fft, mic_mfma, pilot_fft, mic_yic,
 * pilot_fuse, mic2.  Unknown names return DSCE_EINVAL. */
int dsce_set_option(dsce_ctx* ctx, const char* name, int64_t value);
int dsce_get_option(dsce_ctx* ctx, const char* name, int64_t* value);

/* ---- measurement -------------------------------------------------------- */
/* When enabled, dsce_run records HIP events around every launch of each kernel
 * on the stream it runs on; dsce_kernel_time returns (launches, total ms).
 * "ic_stages" is the span of the FFT-form OFDM IC group (k_pic_fft,
 * k_mic_pilot, k_mic_data, in sequence on the context's stream). */
int dsce_enable_timing(dsce_ctx* ctx, int32_t enable);
int dsce_kernel_time(dsce_ctx* ctx, const char* kernel, int64_t* launches, double* total_ms);
/* Algorithmic work of one realisation of a scheme (support-aware): complex
 * multiply-accumulates of the MMSE contraction kernel over W's off-diagonal
 * (row, column) pairs (including, when the last dsce_run fused the MMSE stage
 * into it, the diag(D_hat) = Wd hP products) and the number of W bytes streamed
 * per contraction launch. */
int dsce_work_model(dsce_ctx* ctx, int32_t scheme_id, double* wcontract_cmac_per_rep, double* w_bytes_per_snr);
/* Algorithmic work per realisation of one timed kernel group (the names of
 * dsce_kernel_time) as configured by the last dsce_run, summed over the
 * schemes that ran it: flops (8 per complex multiply-accumulate, 5 n log2 n per
 * n-point DFT; transcendentals and RNG integer work not counted) and the
 * compulsory HBM bytes (each operand read once per realisation / unit, each
 * result written once).  Modelled: the FFT-form OFDM chain (k_jakes, tx,
 * rx_front, perfect_ic, k_mic_pilot, k_mic_data, and ic_stages = the sum of the
 * last three), the polyphase perfect-CSI
 * passes (perfect_ic of FBMC / L = 48 OFDM) and the W contraction (k_wcontract);
 * 0 = not modelled for the path that ran.  DESIGN.md section 4
 * lists the per-unit formulas. */
int dsce_kernel_work(dsce_ctx* ctx, const char* kernel, double* flops_per_rep, double* bytes_per_rep);
/* The guard of the structured MMSE IC (D_hat = Q' H_hat G, DSCE_PATH_MIC_FFT),
 * evaluated at dsce_build_mmse: out[0] = worst over the (variant, SNR) slices of
 * max |Q' H_hat G - W_thr| / (rtol max |W|) over every entry the IC uses, with
 * the slice's rounding bar rtol = min(1e-9, max(1e-11, 4e-16 ||R||_1
 * ||pinv(R)||_1)) (the path is kept iff <= 1), out[1] = the largest absolute
 * deviation, out[2] = the largest |W|, out[3] = the largest rtol of the slices.
 * out[0..2] = -1 when the scheme is not eligible (the W contraction runs).
 * The low-rank form of its tap operator (Bv = T Bz, T_k the J0 kernel summed
 * over pilot symbol k's window; option mic_lr): out[4] = max |Bv - T Bz| /
 * max |Bv| of the fit (-1: not attempted), out[5] = 1 if the operator was
 * built and kept (eligible), else 0 — a run uses it only with the option
 * mic_lr = 1, which DSCE_PATH_MIC_LR of dsce_path_info reports after the
 * run — out[6] = the worst slice's deviation over its rounding
 * bar min(1e-9, max(1e-13, 4e-16 ||R||_1 ||pinv(R)||_1)) max |Bv| (the operator
 * is kept iff <= 1). */
int dsce_structured_check(dsce_ctx* ctx, int32_t scheme_id, double* out7);
/* Measured FP64 matrix-core peak of the context's GPU: back-to-back
 * v_mfma_f64_16x16x4_f64 on independent accumulators, 8 waves per SIMD,
 * best of 3 timed launches (TFLOP/s). */
int dsce_fp64_mfma_peak(dsce_ctx* ctx, double* tflops);

#ifdef __cplusplus
}
#endif

#endif /* DSCE_H */
