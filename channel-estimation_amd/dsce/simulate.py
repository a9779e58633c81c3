"""Command-line Monte-Carlo run: the reference script's loop and plots
(DoublySelectiveChannelEstimation.m:350-631) on one MI355X, or sharded over the
GPUs of a node (one process per GPU, one all-reduce of the counters and MSE
sums — SURVEY §8e; bit-identical counts for any number of ranks).  Two shard
axes: realisations (contiguous slices, the default) or SNR points (--shard snr:
each rank builds the estimator for its own SNR points only, so the setup is
split too; the noise keeps the sweep's SNR index through the engine's snr_base
option):

    python -m dsce.simulate --config default --reps 4096 --out run.json --figures figs/
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m dsce.simulate --config c5 --reps 10048 --out c5.json     # BASELINE config 5
    python -m dsce.simulate --config c5 --devices 0,1,2,3,4,5,6,7   # one process, one multi-device
                                                                    # context (dsce_create_multi: the
                                                                    # in-library RCCL all-reduce)
    python -m dsce.simulate --config paper --checkpoint ck.json --stop-after 4096   # time-boxed slot
    python -m dsce.simulate --config paper --checkpoint ck.json --resume --out paper.json

Checkpoint / resume (the reference has none): --checkpoint
writes the int64 counters, the MSE sums and the next realisation after every
batch (atomically, one file per rank).  The streams are keyed by the global
realisation index, so a resumed run's counts equal an uninterrupted run's bit
for bit.

Progress lines mirror the script's `disp` (script:567); results go through
dsce.results (JSON [+ NPZ], Figures 2-5)."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--config", default="default", help="default (C2-C4) | c5 | paper | doubly_flat (config 1)")
    ap.add_argument("--schemes", default="fbmc_aux,fbmc_cod,ofdm")
    ap.add_argument("--reps", type=int, default=None, help="realisations (any count; default: the config's NrRepetitions)")
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--seed", type=int, default=0x5EED0000)
    ap.add_argument("--out", default=None, help="result JSON")
    ap.add_argument("--npz", action="store_true")
    ap.add_argument("--figures", default=None, help="directory for Figure2-5.png")
    ap.add_argument("--mse", action="store_true", help="also accumulate the channel-estimation NMSE per stage")
    ap.add_argument("--interpolation", default="linear",
                    choices=("linear", "nearest", "natural", "FullAverage"),
                    help="doubly_flat: PSACE interpolation method (the script uses 'linear')")
    ap.add_argument("--shard", choices=("reps", "snr"), default="reps",
                    help="multi-rank split: realisation slices (default) or SNR points")
    ap.add_argument("--devices", default=None,
                    help="comma-separated HIP devices of ONE multi-device context (dsce_create_multi, ABI 7): "
                         "the engine shards the realisations and all-reduces the counters itself (RCCL)")
    ap.add_argument("--checkpoint", default=None,
                    help="JSON checkpoint written after every batch (counters, MSE sums, next realisation); "
                         "one file per rank under a launcher (.rankR suffix)")
    ap.add_argument("--resume", action="store_true", help="continue from --checkpoint if it exists")
    ap.add_argument("--stop-after", type=int, default=None,
                    help="process at most this many realisations (per rank) in this invocation, then leave "
                         "the checkpoint for --resume (needs --checkpoint)")
    ap.add_argument("--rate", choices=("exact", "maxlog"), default=None,
                    help="also the BICM rate per scheme, SNR point and IC stage from the demapper's LLRs "
                         "(exact, or max-log: the mismatched-decoder rate), summed on the GPU (dsce_run_soft)")
    ap.add_argument("--calibrate", action="store_true",
                    help="with --rate: measure the demapper noise ratio rho per SNR point, stage and data symbol "
                         "over the same realisations (dsce_run_calib), for the MMSE and the perfect-CSI branch, "
                         "scale pn_eff by it (dsce_set_llr_scale, dsce_set_llr_scale_perf) and "
                         "report the rate of the scaled LLRs too.  rho is in-sample: the calibrated rate is biased "
                         "upward by O(1 / reps), so a sweep wants thousands of realisations")
    ap.add_argument("--coded", choices=("1/2", "2/3", "3/4", "5/6"), default=None, metavar="RATE",
                    help="also the coded bit and frame error rate per scheme, SNR point and IC stage: the K = 7 "
                         "convolutional code (133, 171) punctured to RATE (1/2, 2/3, 3/4, 5/6), one codeword per "
                         "realisation over a random interleaver, decoded on the GPU from the demapper's LLRs "
                         "(dsce_run_coded; exact LLRs, or --rate's method), MMSE and perfect-CSI branch.  With "
                         "--calibrate it runs after the scale tables are installed")
    ap.add_argument("--coded-interleaver", type=int, default=7, metavar="SEED",
                    help="with --coded: the interleaver is numpy.random.RandomState(SEED).permutation(ND m)")
    ap.add_argument("--ldpc", choices=("1/2", "2/3", "3/4", "5/6"), default=None, metavar="RATE",
                    help="also the LDPC-coded bit and frame error rate and the mean decoder iterations per scheme, "
                         "SNR point and IC stage: a systematic repeat-accumulate code of RATE over the ND m slots "
                         "(dsce.coding.make_ldpc), one codeword per realisation, decoded on the GPU by normalised "
                         "min-sum with early stop from the demapper's LLRs (dsce_run_ldpc; exact LLRs, or --rate's "
                         "method), MMSE and perfect-CSI branch.  Runs after --calibrate's tables and after --coded")
    ap.add_argument("--ldpc-iters", type=int, default=30, metavar="N", help="with --ldpc: the iteration cap (1 .. 100)")
    ap.add_argument("--ldpc-alpha", type=float, default=0.75, metavar="A",
                    help="with --ldpc: the min-sum normalisation, 0 < A <= 1")
    ap.add_argument("--ldpc-seed", type=int, default=7, metavar="S",
                    help="with --ldpc: the code is drawn from numpy.random.RandomState(S)")
    ap.add_argument("--ldpc-schedule", choices=("flooding", "layered"), default=None,
                    help="with --ldpc: flooding (the default; dsce_run_ldpc) or layered over the first-fit layers of "
                         "dsce.coding.make_layers (dsce_run_ldpc_layered): the same error rate in fewer iterations")
    ap.add_argument("--ldpc-fixed", default=None, metavar="QCH,QMSG,QAPP",
                    help="with --ldpc: also decode in fixed point (dsce_run_ldpc_fixed) with these word lengths in bits "
                         "of the channel values, the messages and the a-posteriori sums, a real codeword drawn from "
                         "--ldpc-seed (dsce.coding.ldpc_encode); results under ldpc[scheme]['fixed'] beside the fp64 ones")
    ap.add_argument("--ldpc-scale", type=float, default=None, metavar="S",
                    help="with --ldpc-fixed (required): quantiser steps per LLR unit; the channel clip is "
                         "(2^(QCH-1) - 1) / S")
    ap.add_argument("--ldpc-offset", type=int, default=1, metavar="B", help="with --ldpc-fixed: the offset beta (default 1)")
    ap.add_argument("--ldpc-alpha-q", default="1/2^0", metavar="NUM/2^SH",
                    help="with --ldpc-fixed: the normalisation NUM / 2^SH, rounded half up (default 1/2^0: none)")
    a = ap.parse_args(argv)
    if a.ldpc_schedule and not a.ldpc:
        raise SystemExit("--ldpc-schedule needs --ldpc")
    ldpc_fx = None
    if a.ldpc_fixed is not None or a.ldpc_scale is not None:
        if not a.ldpc:
            raise SystemExit("--ldpc-fixed / --ldpc-scale need --ldpc")
        if a.ldpc_fixed is None or a.ldpc_scale is None:
            raise SystemExit("--ldpc-fixed and --ldpc-scale go together")
        if a.ldpc_schedule == "layered":
            raise SystemExit("--ldpc-fixed cannot be combined with --ldpc-schedule layered (the fixed-point decoder has "
                             "the flooding schedule)")
        import re
        words = re.fullmatch(r"(\d+),(\d+),(\d+)", a.ldpc_fixed.strip())
        if not words:
            raise SystemExit("--ldpc-fixed takes three word lengths, QCH,QMSG,QAPP")
        alpha_q = re.fullmatch(r"(\d+)/2\^(\d+)", a.ldpc_alpha_q.strip())
        if not alpha_q:
            raise SystemExit("--ldpc-alpha-q takes NUM/2^SH, for instance 3/2^2")
        from dsce.coding import make_fixed
        try:
            ldpc_fx = make_fixed(*[int(x) for x in words.groups()], scale=a.ldpc_scale, alpha_num=int(alpha_q.group(1)),
                                 alpha_shift=int(alpha_q.group(2)), beta=a.ldpc_offset)
        except ValueError as e:
            raise SystemExit("--ldpc-fixed: %s" % e)
    if (a.resume or a.stop_after is not None) and not a.checkpoint:
        raise SystemExit("--resume / --stop-after need --checkpoint")
    if a.calibrate and not a.rate:
        raise SystemExit("--calibrate needs --rate")
    if a.rate:
        # the rate pass is one plain sweep of the rank's realisations after the counters
        for on, what in ((a.checkpoint, "--checkpoint (the rate sums are not checkpointed)"),
                         (a.shard == "snr", "--shard snr (the rate pass runs every SNR point of the engine)"),
                         (a.devices, "--devices (dsce_run_soft is member 0's on a multi-device context)"),
                         (a.config == "doubly_flat", "--config doubly_flat (its own simulator)")):
            if on:
                raise SystemExit("--rate cannot be combined with " + what)
    if a.coded:
        # like the rate pass: one plain sweep of the rank's realisations after the counters
        for on, what in ((a.checkpoint, "--checkpoint (the coded counts are not checkpointed)"),
                         (a.shard == "snr", "--shard snr (the coded pass runs every SNR point of the engine)"),
                         (a.devices, "--devices (dsce_run_coded is member 0's on a multi-device context)"),
                         (a.config == "doubly_flat", "--config doubly_flat (its own simulator)")):
            if on:
                raise SystemExit("--coded cannot be combined with " + what)
    if a.ldpc:
        # like the coded pass: one plain sweep of the rank's realisations after the counters
        for on, what in ((a.checkpoint, "--checkpoint (the LDPC counts are not checkpointed)"),
                         (a.shard == "snr", "--shard snr (the LDPC pass runs every SNR point of the engine)"),
                         (a.devices, "--devices (dsce_run_ldpc is member 0's on a multi-device context)"),
                         (a.config == "doubly_flat", "--config doubly_flat (its own simulator)")):
            if on:
                raise SystemExit("--ldpc cannot be combined with " + what)
        if not 1 <= a.ldpc_iters <= 100:
            raise SystemExit("--ldpc-iters must be 1 .. 100")
        if not 0.0 < a.ldpc_alpha <= 1.0:
            raise SystemExit("--ldpc-alpha must be in (0, 1]")

    from dsce import results
    from dsce.configs import build_setup
    from dsce.engine import build_engine

    if a.config == "doubly_flat":
        return _doubly_flat(a)

    from dsce.parallel import allreduce_counts, shard_range

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    device = 0
    # under a launcher (torch.distributed.run sets WORLD_SIZE) the process group
    # and the all-reduce run at every world size, 1 included: the RCCL path of
    # the counters is the same code with one rank or eight
    distributed = "WORLD_SIZE" in os.environ
    devices = [int(d) for d in a.devices.split(",")] if a.devices else None
    if devices and distributed:
        raise SystemExit("--devices is the single-process multi-device path; do not combine it with a launcher")
    if distributed:
        import torch
        import torch.distributed as dist
        # DSCE_DIST_BACKEND=gloo rehearses on a one-GPU box (ranks share the device)
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count())
        torch.cuda.set_device(device)
        dist.init_process_group(os.environ.get("DSCE_DIST_BACKEND", "nccl"))
    names = tuple(a.schemes.split(","))
    from dsce.engine import gpu_tx
    S = build_setup(a.config, schemes=names, tx=gpu_tx(devices[0] if devices else device))   # G / Q on the GPU (row f1)
    reps = a.reps if a.reps is not None else S.n_repetitions    # script:19 / :44, exactly (no rounding)
    if reps < 1:
        raise SystemExit("--reps must be >= 1")
    nsnr = len(S.snr_db)
    if a.shard == "snr":
        # SNR points [s0, s0 + ns) on this rank, every realisation
        s0, ns = shard_range(0, nsnr, world, rank, align=1)
        first, mine = 0, (reps if ns else 0)
        Sr = _snr_subset(S, s0, ns) if ns else None
        options = {"snr_base": s0}
    else:
        s0, ns = 0, nsnr
        first, mine = shard_range(0, reps, world, rank)
        Sr, options = S, {}
    nst = S.n_iter + 1
    counts = np.zeros((len(names), 2, 2, nsnr, nst), dtype=np.int64)
    err = np.zeros((len(names), nsnr, nst))
    pw = np.zeros((len(names), nsnr))
    loss_e = np.zeros((len(names), nsnr, nst, 2))
    loss_p = np.zeros((len(names), nsnr, 2))
    loss_pi = np.zeros_like(loss_e)                  # the perfect-CSI branch at every stage (DSCE_LLR_PERFECT)
    bits, rate_s = None, 0.0
    # --calibrate: the ratio sums and the losses of the scaled LLRs
    n_data = [int(S.schemes[s].n_data) for s in names]
    ratio_e = [np.zeros((nsnr, nst, nd)) for nd in n_data]
    ratio_p = [np.zeros((nsnr, nd)) for nd in n_data]
    closs_e, closs_p = np.zeros_like(loss_e), np.zeros_like(loss_p)
    ratio_pi = [np.zeros((nsnr, nst, nd)) for nd in n_data]
    closs_pi = np.zeros_like(loss_e)
    # --coded: [scheme][branch: mmse, perfect][field: bit_err, frame_err][snr][stage]
    coded = np.zeros((len(names), 2, 2, nsnr, nst), dtype=np.int64)
    codes, coded_s = [], 0.0
    # --ldpc: [scheme][branch: mmse, perfect][field: bit_err, frame_err, iter_sum][snr][stage]
    ldpc = np.zeros((len(names), 2, 3, nsnr, nst), dtype=np.int64)
    ldpc_codes, ldpc_layers, ldpc_s = [], [], 0.0
    ldpcf = np.zeros_like(ldpc)                                # the same from dsce_run_ldpc_fixed (--ldpc-fixed)
    eng = None
    setup_s, t0 = 0.0, time.perf_counter()
    ck_path = None
    if a.checkpoint:
        ck_path = a.checkpoint + (".rank%d" % rank if world > 1 else "")
    ck_key = {"config": a.config, "schemes": list(names), "seed": int(a.seed), "reps": int(reps),
              "shard": a.shard, "world": world, "rank": rank, "first": int(first), "mine": int(mine),
              "mse": bool(a.mse), "snr": [int(s0), int(ns)]}
    done, prior_s = 0, 0.0
    if mine:                                         # a rank with an empty shard contributes zeros
        eng = build_engine(Sr, device=devices or device, batch=max(64, min(a.batch, mine)), options=options)
        setup_s = time.perf_counter() - t0
        sub = np.zeros(eng.counter_shape(), dtype=np.int64)
        e0 = np.zeros((len(names), ns, nst))
        p0 = np.zeros((len(names), ns))
        if a.resume and os.path.exists(ck_path):
            ck = load_checkpoint(ck_path, ck_key)
            done, prior_s = ck["done"], ck["seconds"]
            sub[...] = np.asarray(ck["counts"], dtype=np.int64).reshape(sub.shape)
            if a.mse:
                e0[...] = np.asarray(ck["mse_err"]).reshape(e0.shape)
                p0[...] = np.asarray(ck["mse_pow"]).reshape(p0.shape)
            if rank == 0:
                print("resumed from %s at realisation %d of %d" % (ck_path, first + done, first + mine), flush=True)
        if a.mse:
            eng.enable_mse()
        t0 = time.perf_counter()
        step = min(a.batch * (len(devices) if devices else 1), mine)
        stop = mine if a.stop_after is None else min(mine, done + max(0, a.stop_after))
        start = done
        while done < stop:
            n = min(step, stop - done)
            eng.run(a.seed, first + done, n, sub)
            done += n
            el = time.perf_counter() - t0
            if ck_path:
                e_, p_ = eng.mse() if a.mse else (None, None)
                save_checkpoint(ck_path, ck_key, done, sub, prior_s + el,
                                (e0 + e_, p0 + p_) if a.mse else None)
            if rank == 0:
                print("%d%% Completed! Time Left: %.1f s"
                      % (100 * done // mine, el / (done - start) * (mine - done)), flush=True)
        counts[:, :, :, s0:s0 + ns, :] = sub
        bits = np.array([eng.bits_per_rep(i) for i in range(len(names))])
        if a.mse:
            e_, p_ = eng.mse()
            err[:, s0:s0 + ns, :] = e0 + e_
            pw[:, s0:s0 + ns] = p0 + p_
        if a.rate:
            # one dsce_run_soft pass per scheme over the same realisations, in steps of the batch
            t1 = time.perf_counter()
            for i in range(len(names)):
                out = {"loss_est": loss_e[i], "loss_perf0": loss_p[i]}
                for at in range(0, mine, step):
                    eng.run_soft(i, a.seed, first + at, min(step, mine - at), a.rate, out)
                # one more pass for the perfect-CSI branch
                out = {"loss_est": loss_pi[i]}
                for at in range(0, mine, step):
                    eng.run_soft(i, a.seed, first + at, min(step, mine - at), a.rate, out, branch="perfect")
            if a.calibrate:
                for i in range(len(names)):
                    out = {"ratio_est": ratio_e[i], "ratio_perf0": ratio_p[i]}
                    for at in range(0, mine, step):
                        eng.run_calib(i, a.seed, first + at, min(step, mine - at), out)
                    out = {"ratio_est": ratio_pi[i]}
                    for at in range(0, mine, step):
                        eng.run_calib(i, a.seed, first + at, min(step, mine - at), out, branch="perfect")
            rate_s = time.perf_counter() - t1
    if a.calibrate:
        # rho = ratio / reps over every rank's realisations (the sums are exchanged like the MSE sums; --rate
        # excludes checkpoints, so every rank gets here), installed on every rank, then the rate pass again
        t1 = time.perf_counter()
        if distributed:
            dev = "cuda" if os.environ.get("DSCE_DIST_BACKEND", "nccl") == "nccl" else None
            ratio_e = [allreduce_counts(r, dev) for r in ratio_e]
            ratio_p = [allreduce_counts(r, dev) for r in ratio_p]
            ratio_pi = [allreduce_counts(r, dev) for r in ratio_pi]
        for i in range(len(names) if mine else 0):
            eng.set_llr_scale(i, ratio_e[i] / reps, ratio_p[i] / reps)
            out = {"loss_est": closs_e[i], "loss_perf0": closs_p[i]}
            for at in range(0, mine, step):
                eng.run_soft(i, a.seed, first + at, min(step, mine - at), a.rate, out)
            eng.set_llr_scale_perf(i, ratio_pi[i] / reps)
            out = {"loss_est": closs_pi[i]}
            for at in range(0, mine, step):
                eng.run_soft(i, a.seed, first + at, min(step, mine - at), a.rate, out, branch="perfect")
        rate_s += time.perf_counter() - t1
    if a.coded:
        # one dsce_run_coded pass per scheme and branch over the same realisations, after --calibrate's tables
        from dsce.coding import make_code
        t1 = time.perf_counter()
        for i, s in enumerate(names):
            sc = S.schemes[s]
            codes.append(make_code(int(sc.n_data) * int(sc.bits_per_symbol), a.coded, interleaver=a.coded_interleaver))
            for b, branch in enumerate(("mmse", "perfect") if mine else ()):
                out = {"bit_err": coded[i, b, 0], "frame_err": coded[i, b, 1]}
                for at in range(0, mine, step):
                    eng.run_coded(i, a.seed, first + at, min(step, mine - at), codes[i], a.rate or "exact", out,
                                  branch=branch)
        coded_s = time.perf_counter() - t1
    if a.ldpc:
        # one dsce_run_ldpc pass per scheme and branch over the same realisations, after --coded
        from dsce.coding import make_layers, make_ldpc
        t1 = time.perf_counter()
        for i, s in enumerate(names):
            sc = S.schemes[s]
            ldpc_codes.append(make_ldpc(int(sc.n_data) * int(sc.bits_per_symbol), a.ldpc, seed=a.ldpc_seed,
                                        max_iter=a.ldpc_iters, alpha=a.ldpc_alpha))
            ldpc_layers.append(make_layers(ldpc_codes[i]) if a.ldpc_schedule == "layered" else None)
            for b, branch in enumerate(("mmse", "perfect") if mine else ()):
                out = {"bit_err": ldpc[i, b, 0], "frame_err": ldpc[i, b, 1], "iter_sum": ldpc[i, b, 2]}
                for at in range(0, mine, step):
                    eng.run_ldpc(i, a.seed, first + at, min(step, mine - at), ldpc_codes[i], a.rate or "exact", out,
                                 branch=branch, layers=ldpc_layers[i])
            if ldpc_fx is not None:
                # the transmitted word: information bits from the frozen stream of --ldpc-seed
                from dsce.coding import ldpc_encode
                word = ldpc_encode(np.random.RandomState(a.ldpc_seed).randint(0, 2, ldpc_codes[i].n_info), ldpc_codes[i])
                for b, branch in enumerate(("mmse", "perfect") if mine else ()):
                    out = {"bit_err": ldpcf[i, b, 0], "frame_err": ldpcf[i, b, 1], "iter_sum": ldpcf[i, b, 2]}
                    for at in range(0, mine, step):
                        eng.run_ldpc(i, a.seed, first + at, min(step, mine - at), ldpc_codes[i], a.rate or "exact", out,
                                     branch=branch, fixed=ldpc_fx, codeword=word)
        ldpc_s = time.perf_counter() - t1
    if eng is not None:
        eng.close()
    complete = done >= mine
    if distributed:
        # every rank must take the same branch before the collectives below
        import torch
        import torch.distributed as dist
        f = torch.tensor([0 if complete else 1], dtype=torch.int64)
        if os.environ.get("DSCE_DIST_BACKEND", "nccl") == "nccl":
            f = f.to("cuda")
        dist.all_reduce(f, op=dist.ReduceOp.MAX)
        if int(f.item()):
            complete = False
    if not complete:
        if rank == 0:
            print("stopped at realisation %d of %d; resume with --checkpoint %s --resume"
                  % (first + done, first + mine, a.checkpoint), flush=True)
        if distributed:
            dist.destroy_process_group()
        return 0
    # "seconds" is the counter loop's: the rate pass is timed on its own
    extra = {"setup_s": setup_s, "seconds": prior_s + time.perf_counter() - t0 - rate_s - coded_s - ldpc_s, "ranks": world,
             "shard": a.shard}
    if a.rate:
        extra["bicm_rate_seconds"] = rate_s
    if ck_path and a.resume:
        extra["resumed"] = True
    if devices:
        extra["devices"] = devices
    if distributed:
        dev = "cuda" if os.environ.get("DSCE_DIST_BACKEND", "nccl") == "nccl" else None
        info = {}
        counts = allreduce_counts(counts, dev, info)              # the one exchange
        extra["allreduce"] = info
        if a.mse:
            err = allreduce_counts(err, dev)
            pw = allreduce_counts(pw, dev)
        if a.rate:
            loss_e = allreduce_counts(loss_e, dev)
            loss_p = allreduce_counts(loss_p, dev)
            loss_pi = allreduce_counts(loss_pi, dev)
        if a.coded:
            coded = allreduce_counts(coded, dev)
        if a.ldpc:
            ldpc = allreduce_counts(ldpc, dev)
            if ldpc_fx is not None:
                ldpcf = allreduce_counts(ldpcf, dev)
        if a.calibrate:
            closs_e = allreduce_counts(closs_e, dev)
            closs_p = allreduce_counts(closs_p, dev)
            closs_pi = allreduce_counts(closs_pi, dev)
        # bits per realisation are a property of the schemes: every rank with work
        # has them (collective on every rank, so a rank with an empty shard too)
        have = np.array([0 if bits is None else 1], dtype=np.int64)
        b = np.zeros((len(names), 2), dtype=np.int64) if bits is None else np.asarray(bits, dtype=np.int64)
        b = allreduce_counts(b, dev)
        have = allreduce_counts(have, dev)
        bits = b // max(1, int(have[0]))
        import torch
        import torch.distributed as dist
        t = torch.tensor([extra["seconds"]], dtype=torch.float64)
        if dev:
            t = t.to(dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        extra["seconds"] = float(t.item())
    if a.mse:
        extra["nmse"] = {s: (err[i] / pw[i][:, None]).tolist() for i, s in enumerate(names)}
    if a.rate:
        # I = m - loss / (n_rep ND_edge) bits per data symbol (include/dsce.h), both edge classes
        from dsce.results import EDGE
        extra["bicm_rate"] = {}
        for i, s in enumerate(names):
            m = S.schemes[s].bits_per_symbol
            nd = np.asarray(bits[i], dtype=np.float64) / m
            extra["bicm_rate"][s] = {
                "mmse": {e: (m - loss_e[i, :, :, k] / (reps * nd[k])).tolist() for k, e in enumerate(EDGE)},
                "perfect_onetap": {e: (m - loss_p[i, :, k] / (reps * nd[k])).tolist() for k, e in enumerate(EDGE)},
                "perfect_ic": {e: (m - loss_pi[i, :, :, k] / (reps * nd[k])).tolist() for k, e in enumerate(EDGE)},
                "method": a.rate}
            if a.calibrate:
                # the same with pn_eff <- rho pn_eff; noise_ratio: the mean rho over the symbols of each edge class
                cons = np.asarray(S.schemes[s].considered_symbols).astype(bool)
                sel = (np.ones_like(cons), cons)
                extra["bicm_rate"][s].update({
                    "mmse_calibrated": {e: (m - closs_e[i, :, :, k] / (reps * nd[k])).tolist()
                                        for k, e in enumerate(EDGE)},
                    "perfect_onetap_calibrated": {e: (m - closs_p[i, :, k] / (reps * nd[k])).tolist()
                                                  for k, e in enumerate(EDGE)},
                    "perfect_ic_calibrated": {e: (m - closs_pi[i, :, :, k] / (reps * nd[k])).tolist()
                                              for k, e in enumerate(EDGE)},
                    "noise_ratio": {"mmse": {e: (ratio_e[i][:, :, sel[k]].mean(axis=-1) / reps).tolist()
                                             for k, e in enumerate(EDGE)},
                                    "perfect_onetap": {e: (ratio_p[i][:, sel[k]].mean(axis=-1) / reps).tolist()
                                                       for k, e in enumerate(EDGE)},
                                    "perfect_ic": {e: (ratio_pi[i][:, :, sel[k]].mean(axis=-1) / reps).tolist()
                                                   for k, e in enumerate(EDGE)}},
                    "calibration": {"reps": int(reps), "in_sample": True}})
    if a.coded:
        # BER = bit_err / (reps info_bits), FER = frame_err / reps: one codeword per realisation (include/dsce.h)
        extra["coded_seconds"] = coded_s
        extra["coded"] = {}
        for i, s in enumerate(names):
            k = codes[i].n_info
            extra["coded"][s] = {"rate": a.coded, "info_bits": int(k), "steps": int(codes[i].n_steps),
                                 "interleaver": int(a.coded_interleaver), "method": a.rate or "exact",
                                 "calibrated": bool(a.calibrate)}
            for b, branch in enumerate(("mmse", "perfect_ic")):
                extra["coded"][s][branch] = {"ber": (coded[i, b, 0] / (float(reps) * k)).tolist(),
                                             "fer": (coded[i, b, 1] / float(reps)).tolist()}
    if a.ldpc:
        # BER = bit_err / (reps info_bits), FER = frame_err / reps, mean_iter = iter_sum / reps (include/dsce.h)
        extra["ldpc_seconds"] = ldpc_s
        extra["ldpc"] = {}
        for i, s in enumerate(names):
            c = ldpc_codes[i]
            extra["ldpc"][s] = {"rate": a.ldpc, "info_bits": int(c.n_info), "n_checks": int(c.n_checks),
                                "max_iter": int(c.max_iter), "alpha": float(c.alpha), "seed": int(a.ldpc_seed),
                                "four_cycles": int(c.four_cycles), "method": a.rate or "exact",
                                "calibrated": bool(a.calibrate), "schedule": a.ldpc_schedule or "flooding",
                                "n_layers": ldpc_layers[i][0].size - 1 if ldpc_layers[i] else None}
            for b, branch in enumerate(("mmse", "perfect_ic")):
                extra["ldpc"][s][branch] = {"ber": (ldpc[i, b, 0] / (float(reps) * c.n_info)).tolist(),
                                            "fer": (ldpc[i, b, 1] / float(reps)).tolist(),
                                            "mean_iter": (ldpc[i, b, 2] / float(reps)).tolist()}
            if ldpc_fx is not None:
                C = (1 << (ldpc_fx.q_ch - 1)) - 1
                extra["ldpc"][s]["fixed"] = dict(ldpc_fx._asdict(), clip=C / ldpc_fx.scale, codeword="ldpc_encode of "
                                                 "RandomState(seed).randint(0, 2, info_bits)")
                for b, branch in enumerate(("mmse", "perfect_ic")):
                    extra["ldpc"][s]["fixed"][branch] = {"ber": (ldpcf[i, b, 0] / (float(reps) * c.n_info)).tolist(),
                                                         "fer": (ldpcf[i, b, 1] / float(reps)).tolist(),
                                                         "mean_iter": (ldpcf[i, b, 2] / float(reps)).tolist()}
    extra["realisations_per_s"] = reps / extra["seconds"]
    res = results.make(S, names, counts, bits, reps, a.seed, extra=extra)
    if rank != 0:
        if distributed:
            dist.destroy_process_group()
        return 0
    if a.out:
        results.save(a.out, res, npz=a.npz)
    if a.figures:
        os.makedirs(a.figures, exist_ok=True)
        for f in results.figures(res, a.figures):
            print("wrote", f)
    k = len(S.snr_db) - 1
    summary = {s: {"snr_db": float(S.snr_db[k]),
                   "ber_ic_mmse": float(res["ber"][s]["mmse"]["all"][k][-1]),
                   "ber_onetap_mmse": float(res["ber"][s]["mmse"]["all"][k][0])} for s in names}
    print(json.dumps(summary))
    if a.rate:
        print(json.dumps({s: {"snr_db": float(S.snr_db[k]), "method": a.rate,
                              "bicm_rate_ic_mmse": r["mmse"]["all"][k][-1],
                              "bicm_rate_onetap_mmse": r["mmse"]["all"][k][0],
                              "bicm_rate_onetap_perfect": r["perfect_onetap"]["all"][k],
                              "bicm_rate_ic_perfect": r["perfect_ic"]["all"][k][-1],
                              **({"bicm_rate_ic_mmse_calibrated": r["mmse_calibrated"]["all"][k][-1]}
                                 if a.calibrate else {})}
                          for s, r in extra["bicm_rate"].items()}))
    if a.coded:
        print(json.dumps({s: {"snr_db": float(S.snr_db[k]), "rate": r["rate"], "info_bits": r["info_bits"],
                              "coded_ber_ic_mmse": r["mmse"]["ber"][k][-1],
                              "coded_ber_onetap_mmse": r["mmse"]["ber"][k][0],
                              "coded_fer_ic_mmse": r["mmse"]["fer"][k][-1],
                              "coded_ber_ic_perfect": r["perfect_ic"]["ber"][k][-1]}
                          for s, r in extra["coded"].items()}))
    if a.ldpc:
        print(json.dumps({s: {"snr_db": float(S.snr_db[k]), "rate": r["rate"], "info_bits": r["info_bits"],
                              "ldpc_ber_ic_mmse": r["mmse"]["ber"][k][-1],
                              "ldpc_ber_onetap_mmse": r["mmse"]["ber"][k][0],
                              "ldpc_fer_ic_mmse": r["mmse"]["fer"][k][-1],
                              "ldpc_mean_iter_ic_mmse": r["mmse"]["mean_iter"][k][-1],
                              "ldpc_ber_ic_perfect": r["perfect_ic"]["ber"][k][-1]}
                          for s, r in extra["ldpc"].items()}))
    if distributed:
        dist.destroy_process_group()
    return 0


CHECKPOINT_VERSION = 1


def save_checkpoint(path, key, done, counts, seconds, mse=None):
    """Write the run state atomically (a temporary file, then os.replace): a
    crash while writing leaves the previous checkpoint intact."""
    d = {"version": CHECKPOINT_VERSION, "key": key, "done": int(done), "seconds": float(seconds),
         "counts": np.asarray(counts, dtype=np.int64).ravel().tolist()}
    if mse is not None:
        d["mse_err"] = np.asarray(mse[0]).ravel().tolist()
        d["mse_pow"] = np.asarray(mse[1]).ravel().tolist()
    tmp = path + ".tmp"
    with open(tmp, "w") as f:
        json.dump(d, f)
    os.replace(tmp, path)


def load_checkpoint(path, key):
    """The checkpoint at `path` if it belongs to this run (same configuration,
    schemes, seed, realisation count, shard and rank); anything else is an
    error, never a silent restart or a mixed result."""
    with open(path) as f:
        d = json.load(f)
    if d.get("version") != CHECKPOINT_VERSION:
        raise SystemExit("checkpoint %s: version %r, expected %d" % (path, d.get("version"), CHECKPOINT_VERSION))
    if d.get("key") != key:
        diff = sorted(k for k in set(key) | set(d.get("key", {})) if d.get("key", {}).get(k) != key.get(k))
        raise SystemExit("checkpoint %s belongs to another run (differs in %s)" % (path, ", ".join(diff)))
    if not 0 <= int(d["done"]) <= key["mine"]:
        raise SystemExit("checkpoint %s: realisation count out of range" % path)
    return d


def _snr_subset(S, s0, ns):
    """The setup namespace with SNR points [s0, s0 + ns) only (pn_time, snr_db)."""
    import copy
    T = copy.copy(S)
    T.pn_time = np.asarray(S.pn_time)[s0:s0 + ns]
    T.snr_db = np.asarray(S.snr_db)[s0:s0 + ns]
    return T


def _doubly_flat(a):
    """SimpleVersion_DoublyFlat.m:89-195 (BASELINE config 1) on one GPU."""
    from dsce import results
    from dsce.doubly_flat import DoublyFlatSim

    from dsce.configs import build_doubly_flat_setup
    t0 = time.perf_counter()
    sim = DoublyFlatSim(build_doubly_flat_setup(interpolation=a.interpolation), batch=a.batch)
    setup_s = time.perf_counter() - t0
    S = sim.setup
    reps = a.reps if a.reps is not None else S.n_repetitions    # SimpleVersion_DoublyFlat.m:13, exactly
    if reps < 1:
        raise SystemExit("--reps must be >= 1")
    t0 = time.perf_counter()
    counts = sim.run(a.seed, 0, reps)
    secs = time.perf_counter() - t0
    q = S.schemes["ofdm"].const
    snr_f = np.arange(S.snr_db.min(), S.snr_db.max() + 0.25, 0.5)                     # :180
    theory = _theory(snr_f, q.SymbolMapping, q.BitMapping)
    res = results.doubly_flat_result(sim, counts, reps, a.seed, (snr_f, theory),
                                     extra={"setup_s": setup_s, "seconds": secs,
                                            "realisations_per_s": reps * len(S.snr_db) / secs})
    if a.out:
        results.save(a.out, res)
    if a.figures:
        os.makedirs(a.figures, exist_ok=True)
        print("wrote", results.doubly_flat_figure(res, os.path.join(a.figures, "DoublyFlat.png")))
    print(json.dumps({k: [round(x, 6) for x in v] for k, v in res["ber"].items()}))
    sim.close()
    return 0


def _theory(snr_db, symbols, bitmap):
    """Theory/BitErrorProbabilityDoublyFlatRayleigh.m (host restatement in the
    product package: the plotted reference curve, not a checker)."""
    from dsce.theory import bit_error_probability_doubly_flat_rayleigh
    return bit_error_probability_doubly_flat_rayleigh(snr_db, symbols, bitmap)


if __name__ == "__main__":
    sys.exit(main())
