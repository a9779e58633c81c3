// k_stage_fused and k_detect (kernels_mc.hip), included once per mode:
// STAGE_FUSED_KERNEL / STAGE_DETECT_KERNEL are the kernels' names and
// STAGE_FUSED_BULK whether every unit stores its trace (TraceK bulk mode:
// k_stage_fused_bulk, k_detect_bulk) or only TraceK::unit.  Two kernels of one
// text instead of a shared inlined body: as an inlined function the bodies
// compiled to other code than as the kernels themselves (k_stage_fused 96 -> 145
// VGPRs), and the single-unit kernels are what dsce_run launches.

// data-symbol decisions and bit-error counts, grid (U/64, ceil(ND/32))
__global__ void __launch_bounds__(64) STAGE_DETECT_KERNEL(SchemeK sk, StageArgs st, const uint16_t* __restrict__ sidx,
                                                          const double2* __restrict__ e_est,
                                                          const double2* __restrict__ e_perf,
                                                          uint16_t* __restrict__ qe, uint16_t* __restrict__ qp,
                                                          unsigned long long* __restrict__ counters) {
    constexpr bool BULK = STAGE_FUSED_BULK;
    __shared__ SlicerLds slt;
    const bool lds_slicer = sk.nI <= 16 && sk.nQ <= 16;
    if (lds_slicer) slicer_load(slt, sk, threadIdx.x, WAVE);
    __syncthreads();
    const double sI = sk.slI, sQ = sk.slQ;
    const int unit = blockIdx.x * WAVE + threadIdx.x;
    const int snr = st.snr0 + (blockIdx.x * WAVE) / st.R;
    const int rl = unit % st.R;
    const int U = st.U, R = st.R;
    const int i0 = blockIdx.y * DET_CHUNK;
    const int i1 = min(sk.ND, i0 + DET_CHUNK);
    int cnt[4] = {0, 0, 0, 0};
    for (int csi = 0; csi < 2; ++csi) {
        const double2* __restrict__ e = csi == 0 ? e_est : e_perf;
        uint16_t* __restrict__ qo = csi == 0 ? qe : qp;
        for (int i = i0; i < i1; ++i) {
            double2 z;
            if (sk.despread) {                                  // x = P' (y ./ h), script:436 / :520
                const int row = sk.NP + i;
                double2 acc = make_double2(0.0, 0.0);
                // entries in groups of 4, every load of a group issued before its
                // products (one global round trip per group instead of per entry)
                const int j0 = sk.ph_ptr[row], j1 = sk.ph_ptr[row + 1];
                for (int jb = j0; jb < j1; jb += 4) {
                    double2 ev[4], pv[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int jj = min(jb + g, j1 - 1);
                        pv[g] = jb + g < j1 ? sk.ph_val[jj] : make_double2(0.0, 0.0);
                        ev[g] = e[(size_t)sk.ph_col[jj] * U + unit];
                    }
#pragma unroll
                    for (int g = 0; g < 4; ++g) c_fma(acc, pv[g], ev[g]);
                }
                z = acc;
                z = sk.real_detect ? make_double2(z.x / sk.data_div, 0.0)
                                   : make_double2(z.x / sk.data_div, z.y / sk.data_div);
            } else {                                            // x(data positions) ./ sqrt(DPR)
                z = e[(size_t)sk.data_pos[i] * U + unit];
                z = sk.real_detect ? make_double2(z.x / sk.data_div, 0.0)
                                   : make_double2(z.x / sk.data_div, z.y / sk.data_div);
            }
            const int d = lds_slicer ? slice_fast(slt, sk.nI, sk.nQ, z, sI, sQ) : slice(sk, z);
            const int tx = sidx[(size_t)i * R + rl];
            const int ne = __popc((unsigned)(d ^ tx));
            if (st.tr && trace_hit<BULK>(st.tr, unit))
                (csi ? st.tr->dec_p : st.tr->dec_e)[trace_ix<BULK>(st.tr, (size_t)st.stage * st.tr->ND + i, unit)] = d;
            cnt[csi * 2 + 0] += ne;
            if (sk.considered[i]) cnt[csi * 2 + 1] += ne;
            if (!st.last) qo[(size_t)i * U + unit] = (uint16_t)d;
        }
    }
    flush_counts(cnt, counters, (((size_t)st.scheme * 4) * st.nsnr + snr) * st.nstage + st.stage,
                 (size_t)st.nsnr * st.nstage, 2, rl < st.rvalid);
}

template <int NPT, bool PERF, bool MSE>
__global__ void __launch_bounds__(256) STAGE_FUSED_KERNEL(SchemeK sk, StageArgs st, int nrb,
                                                          const double2* __restrict__ Wd,
                                                          const double2* __restrict__ xp,
                                                          const uint16_t* __restrict__ sidx,
                                                          const double2* __restrict__ h,
                                                          const double2* __restrict__ hp, double2* __restrict__ hest,
                                                          uint16_t* __restrict__ qe, uint16_t* __restrict__ qp,
                                                          double2* __restrict__ v, double2* __restrict__ u,
                                                          unsigned long long* __restrict__ counters) {
    constexpr bool BULK = STAGE_FUSED_BULK;
    constexpr int RB = STAGE_RB;
    __shared__ double2 sym[256];
    __shared__ SlicerLds slt;
    __shared__ double2 shp[NPT * 64];                      // the block's 64 units' LS pilot estimates
    __shared__ double2 swd[4 * RB * NPT];                  // diag(W) rows of the block (broadcast reads)
    // Block = 64 units x 4*RB rows (wave w: rows [4 RB blk + w RB, +RB)); the LS
    // pilot estimates of the 64 units go through LDS once for the 4 waves.
    // Work order: row block fastest, then SNR point, then 64-realisation group,
    // so the blocks sharing hP (same units) and h (same realisations) run close
    // together; with xcd_order each XCD (block b runs on XCD b % 8) walks its own
    // contiguous range of that order, keeping the reuse inside one L2.
    int L = blockIdx.x;
    if (st.xcd_order) L = xcd_remap(L, gridDim.x);
    const int rbk = L % nrb;
    int ug = L / nrb;
    if (st.xcd_order) {
        const int nchunk = st.U / st.R, rgs = st.R >> 6;
        ug = (ug % nchunk) * rgs + ug / nchunk;
    }
    // wave index made provably uniform so Wd / row tables become scalar loads
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int U = st.U, R = st.R;
    const int unit = ug * 64 + lane;
    const int snr = st.snr0 + (ug * 64) / R;
    const int rl = unit % R;
    const int r0 = (rbk * 4 + wv) * RB;
    const int nr = max(0, min(RB, sk.LK - r0));
    // every per-row operand of the wave is requested up front (rows past the
    // end / pilot rows read a valid dummy), so their latency overlaps diag(D_hat)
    double2 ye[RB], yp[RB], hh[RB];
    int tx[RB];
    const bool same_y = st.ysrc_p == st.ysrc_e;
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int row = r < nr ? r0 + r : 0;
        const int i = sk.row_data[row];
        const size_t ix = (size_t)row * U + unit;
        ye[r] = st.ysrc_e[ix];
        tx[r] = sidx[(size_t)(i > 0 ? i : 0) * R + rl];
        if (PERF) yp[r] = same_y ? ye[r] : st.ysrc_p[ix];
        if (PERF || MSE) hh[r] = h[(size_t)row * R + rl];
    }
    // per-row scalars of the wave's rows, requested together (no dependent chains)
    int rdat[RB], rcons[RB], rpcol[RB];
    double2 rpval[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        const int row = r < nr ? r0 + r : 0;
        rdat[r] = sk.row_data[row];
        rcons[r] = sk.row_cons[row];
        rpcol[r] = sk.row_pcol[row];
        rpval[r] = sk.row_pval[row];
    }
    {
        // LDS staging: hP of the 64 units, diag(W) rows of the block, tables;
        // every global load is issued before the first LDS write
        constexpr int NW = (4 * RB * NPT + 255) / 256;
        double2 hv[NPT / 4], wv_[NW];
#pragma unroll
        for (int k = 0; k < NPT / 4; ++k) {
            const int i = threadIdx.x + 256 * k;
            hv[k] = hp[(size_t)(i >> 6) * U + ug * 64 + (i & 63)];
        }
        const int rb0 = rbk * 4 * RB;
        const double2* __restrict__ wdb = Wd + ((size_t)st.var * st.nsnr + snr) * (size_t)sk.LK * NPT;
#pragma unroll
        for (int k = 0; k < NW; ++k) {
            const int i = threadIdx.x + 256 * k;
            const int row = rb0 + i / NPT;
            wv_[k] = (i < 4 * RB * NPT && row < sk.LK) ? wdb[(size_t)rb0 * NPT + i] : make_double2(0.0, 0.0);
        }
        stage_tables<256>(sym, slt, sk, threadIdx.x);
#pragma unroll
        for (int k = 0; k < NPT / 4; ++k) shp[threadIdx.x + 256 * k] = hv[k];
#pragma unroll
        for (int k = 0; k < NW; ++k)
            if (threadIdx.x + 256 * k < 4 * RB * NPT) swd[threadIdx.x + 256 * k] = wv_[k];
    }
    __syncthreads();
    if (nr == 0) return;
    const double2* __restrict__ wds = swd + wv * RB * NPT;
    double2 acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = make_double2(0.0, 0.0);
#pragma unroll
    for (int p = 0; p < NPT; ++p) {
        const double2 hv = shp[p * 64 + lane];
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r < nr) c_fma(acc[r], wds[r * NPT + p], hv);
    }
    if (MSE) {
        double me = 0.0, mp = 0.0;
#pragma unroll
        for (int r = 0; r < RB; ++r)
            if (r < nr) {
                const double dx = acc[r].x - hh[r].x, dy = acc[r].y - hh[r].y;
                me += dx * dx + dy * dy;
                mp += hh[r].x * hh[r].x + hh[r].y * hh[r].y;
            }
        flush_mse(me, mp, st.mse_err, st.mse_pow, st.scheme, st.nsnr, snr, st.nstage, st.stage, rl < st.rvalid);
    }
    const double idd = 1.0 / sk.data_div;
    const double sI = sk.slI, sQ = sk.slQ;
    int cnt[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < RB; ++r) {
        if (r < nr) {
            const int row = r0 + r;
            const size_t ix = (size_t)row * U + unit;
            const bool traced = st.tr && trace_hit<BULK>(st.tr, unit);
            if (traced) st.tr->hest[trace_ix<BULK>(st.tr, (size_t)st.stage * st.tr->LK + row, unit)] = acc[r];
            const int i = rdat[r];
            if (i >= 0) {
                const double2 ze = c_div1(ye[r], acc[r]);
                const int de = slice_fast(slt, sk.nI, sk.nQ, sk.real_detect ? make_double2(ze.x * idd, 0.0)
                                                             : make_double2(ze.x * idd, ze.y * idd), sI, sQ);
                const int ne = __popc((unsigned)(de ^ tx[r]));
                const int cons = rcons[r];
                cnt[0] += ne;
                cnt[1] += cons ? ne : 0;
                int dp = 0;
                if (PERF) {
                    const double2 zp = c_div1(yp[r], hh[r]);
                    dp = slice_fast(slt, sk.nI, sk.nQ, sk.real_detect ? make_double2(zp.x * idd, 0.0)
                                                      : make_double2(zp.x * idd, zp.y * idd), sI, sQ);
                    const int np_ = __popc((unsigned)(dp ^ tx[r]));
                    cnt[2] += np_;
                    cnt[3] += cons ? np_ : 0;
                }
                if (traced) {
                    st.tr->dec_e[trace_ix<BULK>(st.tr, (size_t)st.stage * st.tr->ND + i, unit)] = de;
                    if (PERF) st.tr->dec_p[trace_ix<BULK>(st.tr, (size_t)st.stage * st.tr->ND + i, unit)] = dp;
                }
                if (!st.last) {
                    if (sk.p_diag) {
                        const double2 pv = rpval[r];
                        double2 av = make_double2(0.0, 0.0), au = av;
                        if (rpcol[r] >= 0) {
                            c_fma(av, pv, sym[de]);
                            c_fma(au, pv, sym[dp]);
                        }
                        v[ix] = av;
                        if (PERF) u[ix] = au;
                    } else {
                        const size_t qi = (size_t)i * U + unit;
                        qe[qi] = (uint16_t)de;
                        qp[qi] = (uint16_t)dp;
                    }
                }
            } else if (!st.last && sk.p_diag && st.stage == 0) {   // pilot / empty row: constant P xP
                const int kc = rpcol[r];
                double2 av = make_double2(0.0, 0.0);
                if (kc >= 0) c_fma(av, rpval[r], xp[(size_t)kc * R + rl]);
                v[ix] = av;
                u[ix] = av;
            }
        }
    }
    flush_counts(cnt, counters, (((size_t)st.scheme * 4) * st.nsnr + snr) * st.nstage + st.stage,
                 (size_t)st.nsnr * st.nstage, PERF ? 2 : 1, rl < st.rvalid);
}
