"""Labelled channel-estimation data in bulk: per realisation the received grid
y = Q'r, the LS pilot estimates, the MMSE one-tap estimate, the true one-tap
channel h = diag(Q'HG), the pilots and the transmitted data symbols, written by
the engine's export kernel (dsce_export) into NPZ shards:

    python -m dsce.dataset --config default --scheme ofdm --snr-db 10 20 30 --seed 1 \\
           --first-rep 0 --reps 65536 --shard-reps 8192 --dtype complex64 --out data/ofdm

writes data/ofdm-00000.npz, data/ofdm-00001.npz, ...  A set is addressed by
(seed, first_rep): realisation `rep` of a shard is realisation `rep` of
dsce.simulate with the same seed, so any shard can be regenerated exactly.
dsce.dataset.load(prefix) concatenates the shards.

Arrays of a shard (n = realisations of the shard): y, hp_ls, h_est
[n][n_snr][LK | NP], h [n][LK], xp [n][NP] (complex64 or complex128), sym
[n][ND] int32; metadata: config, scheme, snr_db, pn_time, seed, first_rep,
n_rep, dtype, pilot_pos, data_pos, symbols (the constellation), kappa, data_div,
L, K, abi.

--stages adds what the iterative interference cancellation forms, per stage
s = 0 (one-tap) .. n_iter (dsce_export_stages; --n-iter, default 4 as in the
script): hp_ls_stages [n][n_snr][S][NP], h_est_stages and y_ic_stages
[n][n_snr][S][LK], the detected symbol indices dec_est / dec_perf
[n][n_snr][S][ND] int32 of the MMSE and the perfect-CSI branch, and n_iter in
the metadata.  bit_errors(sym, dec) counts their bit errors per (SNR, stage).

--llr exact|maxlog adds the soft outputs of the MMSE branch per stage
(dsce_export_llr; the stage settings of --stages, --n-iter): the demapper input
x_est [n][n_snr][S][ND], its noise power pn_eff (same shape, float32 / float64)
and llr [n][n_snr][S][ND][m], positive = bit 1, and llr_method and n_iter in the
metadata.  --llr-branch mmse|perfect|both (default mmse) chooses the branch:
the perfect-CSI arrays (DSCE_LLR_PERFECT: y_perf of the stage over the true
one-tap channel h) are stored as x_perf, pn_perf and llr_perf, and llr_branch
goes into the metadata."""
from __future__ import annotations

import argparse
import glob
import os
import sys

import numpy as np

DTYPES = ("complex64", "complex128")
FIELDS = ("y", "hp_ls", "h_est", "h", "xp", "sym")
# shard name of each dsce_export_stages field (--stages)
STAGE_NAMES = {"hp_ls": "hp_ls_stages", "h_est": "h_est_stages", "y_ic": "y_ic_stages", "dec_est": "dec_est",
               "dec_perf": "dec_perf"}
STAGE_ARRAYS = tuple(STAGE_NAMES.values())
# dsce_export_llr fields (--llr), under their own names; the method is metadata key "llr_method"
LLR_ARRAYS = ("x_est", "pn_eff", "llr")
# shard name of each dsce_export_llr field of the perfect-CSI branch (--llr-branch perfect | both)
LLR_PERF_NAMES = {"x_est": "x_perf", "pn_eff": "pn_perf", "llr": "llr_perf"}
LLR_PERF_ARRAYS = tuple(LLR_PERF_NAMES.values())
LLR_BRANCHES = ("mmse", "perfect", "both")


def bit_errors(sym, dec, considered=None):
    """Bit errors per (SNR, stage) of the decisions dec [n][n_snr][S][ND] against
    the transmitted symbol indices sym [n][ND]: popcount(sym ^ dec) summed over
    realisations and data symbols (a symbol index is its bit label), over the
    symbols with considered[i] != 0 when `considered` [ND] is given (the
    scheme's no-edge flags).  int64 [n_snr][S]."""
    sym = np.asarray(sym)
    dec = np.asarray(dec)
    if dec.ndim != 4 or sym.shape != (dec.shape[0], dec.shape[3]):
        raise ValueError("sym must be [n][ND] and dec [n][n_snr][S][ND]")
    if (dec < 0).any():
        raise ValueError("dec holds entries that no kernel formed (-1)")
    x = (sym[:, None, None, :].astype(np.int64) ^ dec.astype(np.int64)).astype(np.uint32)
    nb = np.zeros(x.shape, dtype=np.int64)
    while x.any():
        nb += x & 1
        x = x >> 1
    if considered is not None:
        nb = nb * (np.asarray(considered).reshape(1, 1, 1, -1) != 0)
    return nb.sum(axis=(0, 3))


def shard_path(prefix, index):
    return "%s-%05d.npz" % (prefix, index)


def shard_ranges(first_rep, n_rep, shard_reps):
    """[(first, count)] of the shards of [first_rep, first_rep + n_rep): whole
    shards of shard_reps realisations and one ragged last shard."""
    if n_rep < 0 or shard_reps < 1:
        raise ValueError("n_rep must be >= 0 and shard_reps >= 1")
    return [(first_rep + o, min(shard_reps, n_rep - o)) for o in range(0, n_rep, shard_reps)]


def write_shard(path, arrays, meta):
    """One shard: the exported arrays plus the metadata, atomically (a temporary
    file, then os.replace).  meta must carry first_rep and n_rep."""
    n = int(meta["n_rep"])
    for k, a in arrays.items():
        if k not in FIELDS and k not in STAGE_ARRAYS and k not in LLR_ARRAYS and k not in LLR_PERF_ARRAYS:
            raise ValueError("unknown field %r" % k)
        if a.shape[0] != n:
            raise ValueError("field %s holds %d realisations, the shard %d" % (k, a.shape[0], n))
    clash = set(arrays) & set(meta)
    if clash:
        raise ValueError("metadata keys shadow fields: %s" % sorted(clash))
    d = os.path.dirname(path)
    if d:
        os.makedirs(d, exist_ok=True)
    tmp = path + ".tmp.npz"
    np.savez(tmp, fields=np.array(sorted(arrays)), **arrays, **{k: np.asarray(v) for k, v in meta.items()})
    os.replace(tmp, path)
    return path


def read_shard(path):
    """(arrays, meta) of one shard."""
    with np.load(path, allow_pickle=False) as z:
        names = [str(f) for f in z["fields"]]
        arrays = {k: z[k] for k in names}
        meta = {k: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k not in names and k != "fields"}
    return arrays, meta


def load(prefix):
    """Every shard prefix-NNNNN.npz in order, concatenated over realisations:
    (arrays, meta) with meta of the first shard and n_rep the total.  The
    shards must be contiguous in the realisation index."""
    paths = sorted(glob.glob(glob.escape(prefix) + "-[0-9][0-9][0-9][0-9][0-9].npz"))
    if not paths:
        raise FileNotFoundError("no shards %s-NNNNN.npz" % prefix)
    parts, meta, nxt = [], None, None
    for p in paths:
        a, m = read_shard(p)
        if meta is None:
            meta = dict(m)
        elif int(m["first_rep"]) != nxt or int(m["seed"]) != int(meta["seed"]) or sorted(a) != sorted(parts[0]):
            raise ValueError("shard %s does not continue the set (first_rep %d, expected %d)"
                             % (p, int(m["first_rep"]), nxt))
        nxt = int(m["first_rep"]) + int(m["n_rep"])
        parts.append(a)
    arrays = {k: np.concatenate([a[k] for a in parts], axis=0) for k in parts[0]}
    meta["n_rep"] = nxt - int(meta["first_rep"])
    return arrays, meta


def parser():
    ap = argparse.ArgumentParser(prog="python -m dsce.dataset", description=__doc__.splitlines()[0])
    ap.add_argument("--config", default="default", help="default (C2-C4) | c5 | paper")
    ap.add_argument("--scheme", default="ofdm", choices=("ofdm", "fbmc_aux", "fbmc_cod"))
    ap.add_argument("--snr-db", type=float, nargs="+", default=None, help="SNR points (default: the config's)")
    ap.add_argument("--seed", type=int, default=0x5EED0000)
    ap.add_argument("--first-rep", type=int, default=0)
    ap.add_argument("--reps", type=int, required=True, help="realisations (any count)")
    ap.add_argument("--shard-reps", type=int, default=8192, help="realisations per shard file")
    ap.add_argument("--batch", type=int, default=8192, help="realisations per device batch")
    ap.add_argument("--dtype", choices=DTYPES, default="complex64")
    ap.add_argument("--no-mmse", action="store_true", help="skip dsce_build_mmse and the h_est field")
    ap.add_argument("--stages", action="store_true",
                    help="add the per-stage IC arrays (hp_ls_stages, h_est_stages, y_ic_stages, dec_est, dec_perf)")
    ap.add_argument("--llr", choices=("exact", "maxlog"), default=None,
                    help="add the soft outputs of the MMSE branch per stage (x_est, pn_eff, llr)")
    ap.add_argument("--llr-branch", choices=LLR_BRANCHES, default="mmse",
                    help="with --llr: the MMSE branch (x_est, pn_eff, llr), the perfect-CSI branch "
                         "(x_perf, pn_perf, llr_perf) or both")
    ap.add_argument("--n-iter", type=int, default=None, help="IC iterations of --stages / --llr (default 4)")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", required=True, help="shard prefix: writes PREFIX-00000.npz ...")
    return ap


def main(argv=None):
    a = parser().parse_args(argv)
    if a.reps < 1 or a.shard_reps < 1 or a.first_rep < 0:
        raise SystemExit("--reps and --shard-reps must be >= 1, --first-rep >= 0")
    staged = a.stages or a.llr is not None
    if a.n_iter is not None and not staged:
        raise SystemExit("--n-iter belongs to --stages / --llr")
    if staged and a.no_mmse:
        raise SystemExit("--stages / --llr need the MMSE estimator (drop --no-mmse)")
    if a.llr_branch != "mmse" and a.llr is None:
        raise SystemExit("--llr-branch belongs to --llr")
    if a.n_iter is not None and a.n_iter < 0:
        raise SystemExit("--n-iter must be >= 0")

    from dsce.configs import build_setup
    from dsce.engine import ABI_VERSION, build_engine, gpu_tx

    kw = dict(n_iter=4 if a.n_iter is None else a.n_iter) if staged else {}
    S = build_setup(a.config, schemes=(a.scheme,), snr_db=a.snr_db, tx=gpu_tx(a.device), **kw)
    sc = S.schemes[a.scheme]
    eng = build_engine(S, device=a.device, batch=max(64, min(a.batch, a.reps)), mmse=not a.no_mmse)
    fields = tuple(f for f in FIELDS if not (a.no_mmse and f == "h_est"))
    base = dict(config=a.config, scheme=a.scheme, snr_db=np.asarray(S.snr_db, dtype=float),
                pn_time=np.asarray(S.pn_time, dtype=float), seed=int(a.seed), dtype=a.dtype,
                pilot_pos=np.asarray(sc.pilot_pos, dtype=np.int32), data_pos=np.asarray(sc.data_pos, dtype=np.int32),
                symbols=np.asarray(sc.const.SymbolMapping, dtype=np.complex128).ravel(), kappa=float(sc.kappa),
                data_div=float(sc.data_div), L=int(S.L), K=int(sc.LK // S.L), abi=int(ABI_VERSION))
    if staged:
        base["n_iter"] = int(S.n_iter)
    if a.llr is not None:
        base["llr_method"] = a.llr
        if a.llr_branch != "mmse":
            base["llr_branch"] = a.llr_branch
    try:
        for i, (first, n) in enumerate(shard_ranges(a.first_rep, a.reps, a.shard_reps)):
            arrays = eng.export(0, a.seed, first, n, fields=fields, dtype=np.dtype(a.dtype))
            if a.stages:
                st = eng.export_stages(0, a.seed, first, n, dtype=np.dtype(a.dtype))
                arrays.update({STAGE_NAMES[f]: v for f, v in st.items()})
            if a.llr is not None and a.llr_branch in ("mmse", "both"):
                arrays.update(eng.export_llr(0, a.seed, first, n, method=a.llr, dtype=np.dtype(a.dtype)))
            if a.llr is not None and a.llr_branch in ("perfect", "both"):
                pf = eng.export_llr(0, a.seed, first, n, method=a.llr, dtype=np.dtype(a.dtype), branch="perfect")
                arrays.update({LLR_PERF_NAMES[f]: v for f, v in pf.items()})
            print("wrote", write_shard(shard_path(a.out, i), arrays, dict(base, first_rep=int(first), n_rep=int(n))),
                  flush=True)
    finally:
        eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
