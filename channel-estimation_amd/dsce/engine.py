"""ctypes binding of the C-ABI in include/dsce.h (libdsce.so, HIP for gfx950).

This is the Python twin of the MEX gateway described in INTEGRATION.md: it
converts the host objects (dsce.configs.Scheme, dsce.channel.FastFading) into
the plain column-major interleaved-complex buffers of the ABI.  There is no
CPU fallback: if the shared library is missing or no GPU is present the calls
raise.
"""
from __future__ import annotations

import collections
import ctypes as C
import functools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DSCE_LIB", os.path.join(_HERE, "libdsce.so"))

EXPORTED = [
    "dsce_abi_version", "dsce_device_count", "dsce_create", "dsce_destroy", "dsce_last_error",
    "dsce_set_channel", "dsce_set_snr", "dsce_add_scheme", "dsce_build_mmse", "dsce_set_batch", "dsce_run",
    "dsce_bits_per_rep", "dsce_channel_realise", "dsce_get_correlation", "dsce_get_W", "dsce_trace_unit",
    "dsce_enable_timing", "dsce_kernel_time", "dsce_work_model", "dsce_mmse_onetap", "dsce_tx_matrices",
    "dsce_set_noise_slot", "dsce_set_interpolation", "dsce_enable_mse", "dsce_get_mse", "dsce_trace_unit_ex",
    "dsce_scheme_dims", "dsce_path_info", "dsce_set_option", "dsce_get_option", "dsce_fp64_mfma_peak",
    "dsce_kernel_work", "dsce_structured_check", "dsce_create_multi", "dsce_group_info",
    "dsce_transmission_matrix", "dsce_jakes_info", "dsce_export", "dsce_export_stages",
    "dsce_llr_awgn", "dsce_export_llr", "dsce_llr_info", "dsce_run_soft",
    "dsce_run_calib", "dsce_set_llr_scale", "dsce_get_llr_scale",
    "dsce_set_llr_scale_perf", "dsce_get_llr_scale_perf",
    "dsce_run_coded", "dsce_viterbi",
    "dsce_run_ldpc", "dsce_ldpc",
    "dsce_run_ldpc_layered", "dsce_ldpc_layered",
    "dsce_run_ldpc_fixed", "dsce_ldpc_fixed",
]

ABI_VERSION = 10

# dsce_export flags (include/dsce.h DSCE_EXPORT_*)
EXPORT_F32 = 1 << 0
EXPORT_DEVICE = 1 << 1
# dsce_export fields in the order of dsce_export_out
EXPORT_FIELDS = ("y", "hp_ls", "h_est", "h", "xp", "sym")
# dsce_export_stages fields in the order of dsce_export_stages_out
STAGE_FIELDS = ("hp_ls", "h_est", "y_ic", "dec_est", "dec_perf")
# dsce_llr_awgn / dsce_export_llr (include/dsce.h DSCE_LLR_MAXLOG; DSCE_HAS_LLR)
LLR_MAXLOG = 1 << 2
# dsce_export_llr fields in the order of dsce_export_llr_out
LLR_FIELDS = ("x_est", "pn_eff", "llr")
LLR_METHODS = {"exact": 0, "maxlog": LLR_MAXLOG}
# the perfect-CSI branch of export_llr / run_soft / run_calib (DSCE_LLR_PERFECT; DSCE_HAS_LLR_PERFECT)
LLR_PERFECT = 1 << 4
LLR_BRANCHES = {"mmse": 0, "perfect": LLR_PERFECT}

# dsce_jakes_info kernels (include/dsce.h DSCE_JAKES_*)
JAKES_KERNELS = {0: "none", 1: "static", 2: "discrete", 3: "full", 4: "win_rec", 5: "win_mom", 6: "win_grp"}

# dsce_group_info reduce kinds (include/dsce.h DSCE_REDUCE_*)
REDUCE = {0: "none", 1: "rccl", 2: "host"}

# dsce_path_info bits (include/dsce.h DSCE_PATH_*)
PATH_BITS = {
    "wpair3_fused": 1 << 0, "wpair3": 1 << 1, "wpair4m": 1 << 2, "wcontract_valu": 1 << 3, "pic_mfma": 1 << 4,
    "pic_chain": 1 << 5, "pic_passes": 1 << 6, "stage_fused": 1 << 7, "stage_split": 1 << 8, "noise_fused": 1 << 9,
    "pic_fft": 1 << 10, "mic_fft": 1 << 11, "txrx_fft": 1 << 12, "pilot_fused": 1 << 13, "mic_stages": 1 << 14,
    "mic_lr": 1 << 15, "pic_poly": 1 << 16, "wrow3": 1 << 17, "snr_loop": 1 << 18,
}


class ChannelDesc(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_taps", C.c_int32), ("sampling_rate", C.c_double),
                ("max_doppler", C.c_double), ("n_paths", C.c_int32), ("doppler_model", C.c_int32),
                ("pdp_norm", C.POINTER(C.c_double))]


class SchemeDesc(C.Structure):
    _fields_ = [("n_subcarriers", C.c_int32), ("n_symbols", C.c_int32), ("n_tx_symbols", C.c_int32),
                ("n_pilots", C.c_int32), ("n_data", C.c_int32), ("mod_order", C.c_int32),
                ("bits_per_symbol", C.c_int32), ("despread", C.c_int32), ("real_detect", C.c_int32),
                ("bits_slot", C.c_int32), ("pilot_slot", C.c_int32), ("kappa", C.c_double),
                ("data_div", C.c_double), ("G", C.POINTER(C.c_double)), ("Q", C.POINTER(C.c_double)),
                ("P", C.POINTER(C.c_double)), ("pilot_pos", C.POINTER(C.c_int32)),
                ("data_pos", C.POINTER(C.c_int32)), ("considered", C.POINTER(C.c_uint8)),
                ("symbols", C.POINTER(C.c_double))]


class Dims(C.Structure):
    _fields_ = [("n_samples", C.c_int32), ("n_taps", C.c_int32), ("lk", C.c_int32), ("n_pilots", C.c_int32),
                ("n_data", C.c_int32), ("n_tx_symbols", C.c_int32), ("n_schemes", C.c_int32), ("n_snr", C.c_int32),
                ("n_iter", C.c_int32), ("n_counters", C.c_int64)]


class Trace(C.Structure):
    _fields_ = [("y", C.POINTER(C.c_double)), ("h_perfect", C.POINTER(C.c_double)),
                ("hp_stages", C.POINTER(C.c_double)), ("hest_stages", C.POINTER(C.c_double)),
                ("yest_stages", C.POINTER(C.c_double)), ("yperf_stages", C.POINTER(C.c_double)),
                ("dec_est", C.POINTER(C.c_int32)), ("dec_perf", C.POINTER(C.c_int32))]


class ExportOut(C.Structure):
    _fields_ = [("y", C.c_void_p), ("hp_ls", C.c_void_p), ("h_est", C.c_void_p), ("h", C.c_void_p),
                ("xp", C.c_void_p), ("sym", C.POINTER(C.c_int32))]


class ExportStagesOut(C.Structure):
    _fields_ = [("hp_ls", C.c_void_p), ("h_est", C.c_void_p), ("y_ic", C.c_void_p),
                ("dec_est", C.POINTER(C.c_int32)), ("dec_perf", C.POINTER(C.c_int32))]


class ExportLlrOut(C.Structure):
    _fields_ = [("x_est", C.c_void_p), ("pn_eff", C.c_void_p), ("llr", C.c_void_p)]


class SoftOut(C.Structure):
    _fields_ = [("loss_est", C.POINTER(C.c_double)), ("loss_perf0", C.POINTER(C.c_double))]


class CalibOut(C.Structure):
    _fields_ = [("ratio_est", C.POINTER(C.c_double)), ("ratio_perf0", C.POINTER(C.c_double))]


class CodeDesc(C.Structure):
    _fields_ = [("n_steps", C.c_int32), ("terminated", C.c_int32), ("src", C.POINTER(C.c_int32))]


class CodedOut(C.Structure):
    _fields_ = [("bit_err", C.POINTER(C.c_int64)), ("frame_err", C.POINTER(C.c_int64))]


class LdpcDesc(C.Structure):
    _fields_ = [("n_vars", C.c_int32), ("n_checks", C.c_int32), ("row_ptr", C.POINTER(C.c_int32)),
                ("col", C.POINTER(C.c_int32)), ("slot", C.POINTER(C.c_int32)), ("n_info", C.c_int32),
                ("max_iter", C.c_int32), ("alpha", C.c_double), ("early_stop", C.c_int32)]


class LdpcLayers(C.Structure):
    _fields_ = [("n_layers", C.c_int32), ("layer_ptr", C.POINTER(C.c_int32)), ("layer_check", C.POINTER(C.c_int32))]


class LdpcFixedDesc(C.Structure):
    _fields_ = [("scale", C.c_double), ("q_ch", C.c_int32), ("q_msg", C.c_int32), ("q_app", C.c_int32),
                ("alpha_num", C.c_int32), ("alpha_shift", C.c_int32), ("beta", C.c_int32)]


class LdpcOut(C.Structure):
    _fields_ = [("bit_err", C.POINTER(C.c_int64)), ("frame_err", C.POINTER(C.c_int64)),
                ("iter_sum", C.POINTER(C.c_int64))]


class TxDesc(C.Structure):
    _fields_ = [("kind", C.c_int32), ("n_subcarriers", C.c_int32), ("n_symbols", C.c_int32),
                ("n_samples", C.c_int32), ("fft_size", C.c_int32), ("intermediate_bin", C.c_int32),
                ("time_spacing", C.c_int32), ("cyclic_prefix", C.c_int32), ("zero_guard", C.c_int32),
                ("proto_len", C.c_int32), ("norm", C.c_double), ("initial_phase", C.c_double),
                ("rx_scale", C.c_double), ("prototype", C.POINTER(C.c_double))]


_lib = None


def load_library(path=None):
    """Load libdsce.so (raises OSError with a build hint when it is missing)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise OSError("libdsce.so not found at %s — build it with `make -C channel-estimation_amd` "
                      "(or __graft_entry__.build())" % p)
    lib = C.CDLL(p)
    vp = C.c_void_p
    dp = C.POINTER(C.c_double)
    i64p = C.POINTER(C.c_int64)
    lib.dsce_abi_version.restype = C.c_int
    lib.dsce_device_count.argtypes = [C.POINTER(C.c_int)]
    lib.dsce_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.dsce_create_multi.argtypes = [C.POINTER(C.c_int32), C.c_int32, C.POINTER(vp)]
    lib.dsce_group_info.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.dsce_destroy.argtypes = [vp]
    lib.dsce_destroy.restype = C.c_int
    lib.dsce_last_error.argtypes = [vp]
    lib.dsce_last_error.restype = C.c_char_p
    lib.dsce_set_channel.argtypes = [vp, C.POINTER(ChannelDesc)]
    lib.dsce_set_snr.argtypes = [vp, dp, C.c_int32, C.c_int32]
    lib.dsce_add_scheme.argtypes = [vp, C.POINTER(SchemeDesc), C.POINTER(C.c_int32)]
    lib.dsce_build_mmse.argtypes = [vp, C.c_double]
    lib.dsce_set_batch.argtypes = [vp, C.c_int32]
    lib.dsce_run.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, i64p]
    lib.dsce_bits_per_rep.argtypes = [vp, C.c_int32, i64p]
    lib.dsce_channel_realise.argtypes = [vp, C.c_uint64, C.c_uint64, dp]
    lib.dsce_get_correlation.argtypes = [vp, C.c_int32, dp, dp, dp]
    lib.dsce_transmission_matrix.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, dp]
    lib.dsce_get_W.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp]
    lib.dsce_trace_unit.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, dp, dp, dp, dp]
    lib.dsce_enable_timing.argtypes = [vp, C.c_int32]
    lib.dsce_kernel_time.argtypes = [vp, C.c_char_p, i64p, dp]
    lib.dsce_work_model.argtypes = [vp, C.c_int32, dp, dp]
    lib.dsce_mmse_onetap.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, dp, C.c_int32, dp]
    lib.dsce_tx_matrices.argtypes = [vp, C.POINTER(TxDesc), dp, dp]
    lib.dsce_set_noise_slot.argtypes = [vp, C.c_int32, C.c_int32]
    lib.dsce_set_interpolation.argtypes = [vp, C.c_int32, dp]
    lib.dsce_enable_mse.argtypes = [vp, C.c_int32]
    lib.dsce_get_mse.argtypes = [vp, dp, dp]
    lib.dsce_trace_unit_ex.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_int32, C.POINTER(Trace)]
    lib.dsce_scheme_dims.argtypes = [vp, C.c_int32, C.POINTER(Dims)]
    lib.dsce_path_info.argtypes = [vp, C.c_int32, C.POINTER(C.c_uint32)]
    lib.dsce_jakes_info.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.dsce_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.dsce_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
    lib.dsce_fp64_mfma_peak.argtypes = [vp, dp]
    lib.dsce_kernel_work.argtypes = [vp, C.c_char_p, dp, dp]
    lib.dsce_structured_check.argtypes = [vp, C.c_int32, dp]
    lib.dsce_export.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(ExportOut)]
    lib.dsce_export_stages.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                       C.POINTER(ExportStagesOut)]
    lib.dsce_llr_awgn.argtypes = [vp, C.c_int32, C.c_uint32, dp, dp, C.c_int64, C.c_int64, dp]
    lib.dsce_export_llr.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                    C.POINTER(ExportLlrOut)]
    lib.dsce_llr_info.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    lib.dsce_run_soft.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(SoftOut)]
    lib.dsce_run_calib.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(CalibOut)]
    lib.dsce_set_llr_scale.argtypes = [vp, C.c_int32, dp, dp]
    lib.dsce_get_llr_scale.argtypes = [vp, C.c_int32, dp, dp, C.POINTER(C.c_int32)]
    lib.dsce_set_llr_scale_perf.argtypes = [vp, C.c_int32, dp]
    lib.dsce_get_llr_scale_perf.argtypes = [vp, C.c_int32, dp, C.POINTER(C.c_int32)]
    lib.dsce_run_coded.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                   C.POINTER(CodeDesc), C.POINTER(CodedOut)]
    lib.dsce_viterbi.argtypes = [vp, C.POINTER(CodeDesc), C.c_int64, dp, C.c_int64, C.POINTER(C.c_uint8)]
    lib.dsce_run_ldpc.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                  C.POINTER(LdpcDesc), C.POINTER(LdpcOut)]
    lib.dsce_ldpc.argtypes = [vp, C.POINTER(LdpcDesc), C.c_int64, dp, C.c_int64, C.POINTER(C.c_uint8),
                              C.POINTER(C.c_int32)]
    lib.dsce_run_ldpc_layered.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                          C.POINTER(LdpcDesc), C.POINTER(LdpcLayers), C.POINTER(LdpcOut)]
    lib.dsce_ldpc_layered.argtypes = [vp, C.POINTER(LdpcDesc), C.POINTER(LdpcLayers), C.c_int64, dp, C.c_int64,
                                      C.POINTER(C.c_uint8), C.POINTER(C.c_int32)]
    lib.dsce_run_ldpc_fixed.argtypes = [vp, C.c_int32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32,
                                        C.POINTER(LdpcDesc), C.POINTER(LdpcFixedDesc), C.POINTER(C.c_uint8),
                                        C.POINTER(LdpcOut)]
    lib.dsce_ldpc_fixed.argtypes = [vp, C.POINTER(LdpcDesc), C.POINTER(LdpcFixedDesc), C.c_int64, dp, C.c_int64,
                                    C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_int16)]
    for name in EXPORTED:
        fn = getattr(lib, name)
        if name != "dsce_last_error":
            fn.restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def _cplx(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.complex128).reshape(-1, order="F"))
    return a


def _dptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class DsceError(RuntimeError):
    pass


class Engine:
    """One engine context = one GPU + one HIP stream (dsce_create), or, with a
    sequence of devices, one multi-device context (dsce_create_multi, ABI 7):
    every configuration call reaches every member, run() shards the
    realisations over the members and sums their counters with one in-library
    RCCL all-reduce (host sum when a device repeats)."""

    def __init__(self, device=0, lib_path=None):
        self.lib = load_library(lib_path)
        h = C.c_void_p()
        if isinstance(device, (list, tuple, np.ndarray)):
            devs = np.ascontiguousarray(device, dtype=np.int32)
            rc = self.lib.dsce_create_multi(devs.ctypes.data_as(C.POINTER(C.c_int32)), int(devs.size), C.byref(h))
            what = "dsce_create_multi(devices=%s)" % list(devs)
        else:
            rc = self.lib.dsce_create(int(device), C.byref(h))
            what = "dsce_create(device=%d)" % device
        if rc != 0 or not h.value:
            raise DsceError("%s failed with %d (no HIP device?)" % (what, rc))
        self.h = h
        self._keep = []
        self.schemes = []
        self.nsnr = 0
        self.niter = 0
        self.N = None
        self.ntaps = None

    def _chk(self, rc, what):
        if rc != 0:
            msg = self.lib.dsce_last_error(self.h)
            raise DsceError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))

    def close(self):
        """dsce_destroy; raises DsceError when a HIP call of the teardown failed
        (ABI 6; the context is freed either way)."""
        if getattr(self, "h", None) is not None and self.h.value:
            rc = self.lib.dsce_destroy(self.h)
            self.h = None
            if rc != 0:
                raise DsceError("dsce_destroy failed (%d): a HIP call of the teardown failed (see stderr)" % rc)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- configuration -------------------------------------------------------
    def set_channel(self, ff):
        pdp = np.ascontiguousarray(ff.PowerDelayProfileNormalized, dtype=np.float64)
        self._keep.append(pdp)
        d = ChannelDesc(ff.SamplesTotal, pdp.size, ff.SamplingRate, ff.MaximumDopplerShift, ff.Paths,
                        ff.MODELS[ff.DopplerModel], _dptr(pdp))
        self._chk(self.lib.dsce_set_channel(self.h, C.byref(d)), "dsce_set_channel")
        self.N = ff.SamplesTotal
        self.ntaps = pdp.size

    def set_snr(self, pn_time, n_iter):
        pn = np.ascontiguousarray(pn_time, dtype=np.float64)
        self._chk(self.lib.dsce_set_snr(self.h, _dptr(pn), pn.size, int(n_iter)), "dsce_set_snr")
        self.nsnr = pn.size
        self.niter = int(n_iter)

    def add_scheme(self, sc):
        G = _cplx(sc.G)
        Q = _cplx(sc.Q)
        P = _cplx(sc.P)
        pil = np.ascontiguousarray(sc.pilot_pos, dtype=np.int32)
        dat = np.ascontiguousarray(sc.data_pos, dtype=np.int32)
        cons = np.ascontiguousarray(sc.considered_symbols, dtype=np.uint8)
        sym = _cplx(sc.const.SymbolMapping)
        self._keep += [G, Q, P, pil, dat, cons, sym]
        L = sc.extras.get("pilot_matrix").shape[0] if "pilot_matrix" in sc.extras else sc.LK
        d = SchemeDesc(L, sc.LK // L, sc.P.shape[1], sc.n_pilots, sc.n_data, sc.const.ModulationOrder,
                       sc.bits_per_symbol, int(sc.despread), int(sc.real_detect), sc.bits_slot, sc.pilot_slot,
                       sc.kappa, sc.data_div, _dptr(G), _dptr(Q), _dptr(P),
                       pil.ctypes.data_as(C.POINTER(C.c_int32)), dat.ctypes.data_as(C.POINTER(C.c_int32)),
                       cons.ctypes.data_as(C.POINTER(C.c_uint8)), _dptr(sym))
        sid = C.c_int32()
        self._chk(self.lib.dsce_add_scheme(self.h, C.byref(d), C.byref(sid)), "dsce_add_scheme")
        self.schemes.append(sc)
        return sid.value

    def set_noise_slot(self, sid, slot):
        """Schemes of one slot share the AWGN draw (dsce_set_noise_slot)."""
        self._chk(self.lib.dsce_set_noise_slot(self.h, int(sid), int(slot)), "dsce_set_noise_slot")

    def set_interpolation(self, sid, interp):
        """One-tap estimate h_hat = interp @ hP (LK x NP) instead of the MMSE W
        (dsce_set_interpolation; PSACE ChannelInterpolation weights)."""
        sc = self.schemes[sid]
        I = _cplx(np.asarray(interp).reshape(sc.LK, sc.n_pilots))
        self._keep.append(I)
        self._chk(self.lib.dsce_set_interpolation(self.h, int(sid), _dptr(I)), "dsce_set_interpolation")

    def build_mmse(self, zero_threshold=1e-8):
        self._chk(self.lib.dsce_build_mmse(self.h, float(zero_threshold)), "dsce_build_mmse")

    def set_batch(self, reps):
        self._chk(self.lib.dsce_set_batch(self.h, int(reps)), "dsce_set_batch")

    # -- Monte Carlo -----------------------------------------------------------
    def counter_shape(self):
        return (len(self.schemes), 2, 2, self.nsnr, 1 + self.niter)

    def run(self, seed, first_rep, n_rep, counts=None):
        if counts is None:
            counts = np.zeros(self.counter_shape(), dtype=np.int64)
        assert counts.dtype == np.int64 and counts.flags.c_contiguous and counts.shape == self.counter_shape()
        self._chk(self.lib.dsce_run(self.h, int(seed), int(first_rep), int(n_rep),
                                    counts.ctypes.data_as(C.POINTER(C.c_int64))), "dsce_run")
        return counts

    def bits_per_rep(self, sid):
        b = np.zeros(2, dtype=np.int64)
        self._chk(self.lib.dsce_bits_per_rep(self.h, int(sid), b.ctypes.data_as(C.POINTER(C.c_int64))),
                  "dsce_bits_per_rep")
        return b

    # -- setup producers (row f1) ----------------------------------------------
    def tx_matrices(self, mod):
        """(G, Q) of a dsce.modulation.OFDM / FBMC object computed on the GPU:
        G = mod.GetTXMatrix(), Q = mod.GetRXMatrix()' (script:191-195)."""
        from dsce.modulation import FBMC, OFDM
        Nr, Impl, PHY = mod.Nr, mod.Implementation, mod.PHY
        L, K, N = Nr.Subcarriers, Nr.MCSymbols, Nr.SamplesTotal
        proto = None
        if isinstance(mod, OFDM):
            if PHY.TransmitRealSignal:
                raise DsceError("GetTXMatrix is not supported for PHY.TransmitRealSignal == true")
            d = TxDesc(0, L, K, N, Impl.FFTSize, Impl.IntermediateFrequency, Impl.TimeSpacing, Impl.CyclicPrefix,
                       Impl.ZeroGuardSamples, 0, Impl.NormalizationFactor, 0.0,
                       L * PHY.SubcarrierSpacing / PHY.SamplingRate, None)
        elif isinstance(mod, FBMC):
            if PHY.TransmitRealSignal:
                raise DsceError("real-signal FBMC is not supported")
            proto = np.ascontiguousarray(mod.PrototypeFilter.TimeDomain, dtype=np.float64)
            d = TxDesc(1, L, K, N, Impl.FFTSize, Impl.IntermediateFrequency, Impl.TimeSpacing, 0, 0, proto.size,
                       Impl.NormalizationFactor, Impl.InitialPhaseShift, L / (PHY.SamplingRate * PHY.TimeSpacing),
                       _dptr(proto))
        else:
            raise TypeError("OFDM or FBMC object expected")
        G = np.zeros(2 * N * L * K)
        Q = np.zeros(2 * N * L * K)
        self._chk(self.lib.dsce_tx_matrices(self.h, C.byref(d), _dptr(G), _dptr(Q)), "dsce_tx_matrices")
        shape = (N, L * K)
        return (G.view(np.complex128).reshape(shape, order="F"), Q.view(np.complex128).reshape(shape, order="F"))

    # -- probes ----------------------------------------------------------------
    def channel_impulse_response(self, seed, rep):
        out = np.zeros(2 * self.N * self.ntaps)
        self._chk(self.lib.dsce_channel_realise(self.h, int(seed), int(rep), _dptr(out)), "dsce_channel_realise")
        return out.view(np.complex128).reshape(self.N, self.ntaps, order="F")

    def transmission_matrix(self, sid, seed, rep):
        """D = Q^H H G (LK x LK) of realisation `rep` (dsce_transmission_matrix,
        script:381-393)."""
        LK = self.schemes[sid].LK
        out = np.zeros(2 * LK * LK)
        self._chk(self.lib.dsce_transmission_matrix(self.h, int(sid), int(seed), int(rep), _dptr(out)),
                  "dsce_transmission_matrix")
        return out.view(np.complex128).reshape(LK, LK, order="F")

    def correlation(self, sid):
        NP = self.schemes[sid].n_pilots
        rhp = np.zeros(2 * NP * NP)
        rest = np.zeros(2 * self.nsnr * NP * NP)
        rnoi = np.zeros(2 * self.nsnr * NP * NP)
        self._chk(self.lib.dsce_get_correlation(self.h, int(sid), _dptr(rhp), _dptr(rest), _dptr(rnoi)),
                  "dsce_get_correlation")
        f = lambda a, n: a.view(np.complex128).reshape(n, NP, NP).transpose(0, 2, 1)   # column-major NP x NP
        return f(rhp, 1)[0], f(rest, self.nsnr), f(rnoi, self.nsnr)

    def W(self, sid, snr_index, variant=0):
        sc = self.schemes[sid]
        out = np.zeros(2 * sc.LK * sc.LK * sc.n_pilots)
        self._chk(self.lib.dsce_get_W(self.h, int(sid), int(snr_index), int(variant), _dptr(out)), "dsce_get_W")
        return out.view(np.complex128)

    def trace_unit(self, sid, seed, rep, snr_index):
        """Every stage of one (rep, SNR) unit through the same kernels as run()
        (dsce_trace_unit_ex): y, h (= diag D), and per stage hp (LS pilots), hest
        (diag D_hat), yest / yperf (IC inputs; row 0 = y) and the detected symbol
        indices dec_e / dec_p (-1 where the path forms no decision)."""
        d = self.scheme_dims(sid)
        ns, LK, NP, ND = d.n_iter + 1, d.lk, d.n_pilots, d.n_data
        bufs = dict(y=np.zeros(2 * LK), h=np.zeros(2 * LK), hp=np.zeros(2 * ns * NP), hest=np.zeros(2 * ns * LK),
                    yest=np.zeros(2 * ns * LK), yperf=np.zeros(2 * ns * LK))
        dec_e = np.zeros(ns * ND, dtype=np.int32)
        dec_p = np.zeros(ns * ND, dtype=np.int32)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        t = Trace(_dptr(bufs["y"]), _dptr(bufs["h"]), _dptr(bufs["hp"]), _dptr(bufs["hest"]), _dptr(bufs["yest"]),
                  _dptr(bufs["yperf"]), ip(dec_e), ip(dec_p))
        self._chk(self.lib.dsce_trace_unit_ex(self.h, int(sid), int(seed), int(rep), int(snr_index), C.byref(t)),
                  "dsce_trace_unit_ex")
        v = lambda a: a.view(np.complex128)
        return dict(y=v(bufs["y"]), h=v(bufs["h"]), hp=v(bufs["hp"]).reshape(ns, NP),
                    hest=v(bufs["hest"]).reshape(ns, LK), yest=v(bufs["yest"]).reshape(ns, LK),
                    yperf=v(bufs["yperf"]).reshape(ns, LK), dec_e=dec_e.reshape(ns, ND), dec_p=dec_p.reshape(ns, ND))

    # -- bulk exports: dsce_export (ABI 9), dsce_export_stages (ABI 10), dsce_export_llr (DSCE_HAS_LLR)
    def _export_call(self, kind, sid, seed, first_rep, n_rep, flags, ptrs):
        """The entry point of export `kind` (a key of _EXPORTS) on raw addresses:
        ptrs maps a field to where its array starts (host, or device memory with
        EXPORT_DEVICE in flags)."""
        k = _EXPORTS[kind]
        bad = [f for f in ptrs if f not in k.fields]
        if bad:
            raise ValueError("unknown %s field(s) %s (of %s)" % (k.noun, bad, list(k.fields)))
        o = k.struct()
        for f, p in ptrs.items():
            setattr(o, f, C.cast(p, C.POINTER(C.c_int32)) if k.kinds[f] == "int32" else p)
        self._chk(getattr(self.lib, k.entry)(self.h, int(sid), int(seed), int(first_rep), int(n_rep), int(flags),
                                             C.byref(o)), k.entry)

    # the raw-address form per kind, (sid, seed, first_rep, n_rep, flags, ptrs): what the
    # GPU tests' guard-byte wrappers and tools/export_measure.py call
    _export = functools.partialmethod(_export_call, "export")
    _export_stages = functools.partialmethod(_export_call, "stages")
    _export_llr = functools.partialmethod(_export_call, "llr")

    def _bulk_export(self, kind, sid, seed, first_rep, n_rep, fields, arrays, method=None, branch="mmse"):
        """Export `kind` into arrays that `arrays` (_HostArrays or _TorchArrays)
        allocates: a dict field -> array."""
        k = _EXPORTS[kind]
        shapes = k.shapes(self, sid, n_rep)
        out = {f: arrays.empty(shapes[f], k.kinds[f]) for f in fields}
        arrays.ready()
        flags = arrays.flags | (0 if method is None else self._llr_flag(method)) | self._branch_flag(branch)
        self._export_call(kind, sid, seed, first_rep, n_rep, flags, {f: arrays.address(a) for f, a in out.items()})
        return out

    def export_shapes(self, sid, n_rep):
        """Shapes of dsce_export's arrays for n_rep realisations of scheme sid."""
        d = self.scheme_dims(sid)
        n = int(n_rep)
        return dict(y=(n, d.n_snr, d.lk), hp_ls=(n, d.n_snr, d.n_pilots), h_est=(n, d.n_snr, d.lk), h=(n, d.lk),
                    xp=(n, d.n_pilots), sym=(n, d.n_data))

    def export(self, sid, seed, first_rep, n_rep, fields=EXPORT_FIELDS, dtype=np.complex128):
        """Per-realisation data of realisations [first_rep, first_rep + n_rep) of
        scheme sid (dsce_export) as a dict of NumPy arrays: y, hp_ls, h_est
        [n_rep][n_snr][LK | NP], h [n_rep][LK], xp [n_rep][NP] (dtype complex128,
        or complex64: DSCE_EXPORT_F32) and sym [n_rep][ND] int32.  Realisation
        rep is realisation rep of run() with the same seed."""
        return self._bulk_export("export", sid, seed, first_rep, n_rep, fields, _HostArrays(dtype))

    def export_torch(self, sid, seed, first_rep, n_rep, fields=EXPORT_FIELDS, dtype=None, device=None):
        """export() into torch tensors on the context's GPU, written by the export
        kernel itself (DSCE_EXPORT_DEVICE): no host copy.  dtype torch.complex128
        (default) or torch.complex64; sym is torch.int32.  device: the HIP device
        of the context (default: member 0 of group_info()).

        torch and the engine must share one HIP runtime for a pointer of one to
        mean anything to the other.  A torch wheel that bundles its runtime gets
        that when torch is imported before the engine's library is loaded
        (libdsce.so then binds to the runtime torch loaded, like bench.py and
        dsce.simulate under a launcher); the other order leaves torch without a
        usable device, which is reported here."""
        return self._bulk_export("export", sid, seed, first_rep, n_rep, fields,
                                 _TorchArrays(self, "export_torch", dtype, device))

    def export_stages_shapes(self, sid, n_rep):
        """Shapes of dsce_export_stages' arrays for n_rep realisations of scheme sid
        (S = 1 + n_iter stages)."""
        d = self.scheme_dims(sid)
        n, S = int(n_rep), d.n_iter + 1
        return dict(hp_ls=(n, d.n_snr, S, d.n_pilots), h_est=(n, d.n_snr, S, d.lk), y_ic=(n, d.n_snr, S, d.lk),
                    dec_est=(n, d.n_snr, S, d.n_data), dec_perf=(n, d.n_snr, S, d.n_data))

    def export_stages(self, sid, seed, first_rep, n_rep, fields=STAGE_FIELDS, dtype=np.complex128):
        """Per-stage IC data of realisations [first_rep, first_rep + n_rep) of
        scheme sid (dsce_export_stages) as a dict of NumPy arrays, stage 0 = the
        one-tap stage, stage i = IC iteration i: hp_ls [n_rep][n_snr][S][NP], h_est
        and y_ic [n_rep][n_snr][S][LK] (dtype complex128, or complex64:
        DSCE_EXPORT_F32), dec_est / dec_perf [n_rep][n_snr][S][ND] int32 (the
        detected symbol indices of the MMSE and the perfect-CSI branch).  From the
        kernels of run() on its path; realisation rep is realisation rep of run()
        and of export() with the same seed.  NaN / -1: formed by no kernel of the
        path."""
        return self._bulk_export("stages", sid, seed, first_rep, n_rep, fields, _HostArrays(dtype))

    def export_stages_torch(self, sid, seed, first_rep, n_rep, fields=STAGE_FIELDS, dtype=None, device=None):
        """export_stages() into torch tensors on the context's GPU, written by the
        export kernel itself (DSCE_EXPORT_DEVICE); see export_torch for dtype,
        device and the import order of torch and the engine."""
        return self._bulk_export("stages", sid, seed, first_rep, n_rep, fields,
                                 _TorchArrays(self, "export_stages_torch", dtype, device))

    # -- soft outputs (DSCE_HAS_LLR) ----------------------------------------------
    @staticmethod
    def _llr_flag(method):
        if method not in LLR_METHODS:
            raise ValueError("LLR method must be 'exact' or 'maxlog'")
        return LLR_METHODS[method]

    @staticmethod
    def _branch_flag(branch):
        if branch not in LLR_BRANCHES:
            raise ValueError("branch must be 'mmse' or 'perfect'")
        return LLR_BRANCHES[branch]

    def llr_info(self, sid):
        """dict(per_axis, m) of scheme sid's demapper (dsce_llr_info): per_axis =
        every bit of the label depends on one axis of the constellation grid, so
        the LLRs are PAM LLRs per axis; else the full-table form runs."""
        out = (C.c_int32 * 2)()
        self._chk(self.lib.dsce_llr_info(self.h, int(sid), out), "dsce_llr_info")
        return dict(per_axis=bool(out[0]), m=int(out[1]))

    def llr_awgn(self, sid, x, pn, method="exact"):
        """SignalConstellation.LLR_AWGN of scheme sid's constellation on the GPU
        (dsce_llr_awgn): x complex [n], pn a scalar or [n]; returns [n][m] float64,
        positive = bit 1.  The arithmetic of export_llr."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.complex128).reshape(-1))
        pn = np.ascontiguousarray(np.asarray(pn, dtype=np.float64).reshape(-1))
        out = np.zeros((x.size, self.llr_info(sid)["m"]))
        self._chk(self.lib.dsce_llr_awgn(self.h, int(sid), self._llr_flag(method), _dptr(x.view(np.float64)),
                                         _dptr(pn), pn.size, x.size, _dptr(out)), "dsce_llr_awgn")
        return out

    def export_llr_shapes(self, sid, n_rep):
        """Shapes of dsce_export_llr's arrays for n_rep realisations of scheme sid
        (S = 1 + n_iter stages, m bits per symbol)."""
        d = self.scheme_dims(sid)
        n, S = int(n_rep), d.n_iter + 1
        base = (n, d.n_snr, S, d.n_data)
        return dict(x_est=base, pn_eff=base, llr=base + (self.llr_info(sid)["m"],))

    def export_llr(self, sid, seed, first_rep, n_rep, fields=LLR_FIELDS, method="exact", dtype=np.complex128,
                   branch="mmse"):
        """Soft outputs of the MMSE branch (branch 'perfect': of the perfect-CSI
        branch, DSCE_LLR_PERFECT: y_perf of the stage over h = diag(D)) for realisations [first_rep, first_rep +
        n_rep) of scheme sid, every SNR point and stage (dsce_export_llr) as a dict
        of NumPy arrays: the demapper input x_est [n_rep][n_snr][S][ND] (dtype
        complex128, or complex64: DSCE_EXPORT_F32), its noise power pn_eff (same
        shape, float64 / float32) and llr [n_rep][n_snr][S][ND][m], positive = bit
        1, method 'exact' (log-sum-exp) or 'maxlog'.  Realisation rep is
        realisation rep of run(), export() and export_stages() with the same seed."""
        return self._bulk_export("llr", sid, seed, first_rep, n_rep, fields, _HostArrays(dtype), method, branch)

    def export_llr_torch(self, sid, seed, first_rep, n_rep, fields=LLR_FIELDS, method="exact", dtype=None,
                         device=None, branch="mmse"):
        """export_llr() into torch tensors on the context's GPU, written by the
        kernel itself (DSCE_EXPORT_DEVICE); dtype torch.complex128 (x_est; pn_eff
        and llr float64) or torch.complex64 (float32).  See export_torch for
        device and the import order of torch and the engine."""
        return self._bulk_export("llr", sid, seed, first_rep, n_rep, fields,
                                 _TorchArrays(self, "export_llr_torch", dtype, device), method, branch)

    # -- the runs that accumulate on the GPU (run_soft, run_calib, run_coded, run_ldpc) ---
    @staticmethod
    def _acc_out(struct, shapes, dtype, out, default, noun):
        """(struct filled with the pointers of `out`, out) for an accumulating run:
        `out` a dict of C-contiguous `dtype` arrays of `shapes`, or None for zeros
        under the `default` keys; `noun` names the outputs in the messages."""
        if out is None:
            out = {f: np.zeros(shapes[f], dtype=dtype) for f in default}
        o, ptr = struct(), dict(struct._fields_)
        for f, a in out.items():
            if f not in shapes:
                raise ValueError("unknown %s output %r (of %s)" % (noun, f, list(shapes)))
            if not (isinstance(a, np.ndarray) and a.dtype == dtype and a.flags.c_contiguous
                    and a.shape == shapes[f]):
                raise ValueError("%s must be a C-contiguous %s array of shape %s"
                                 % (f, np.dtype(dtype).name, shapes[f]))
            setattr(o, f, a.ctypes.data_as(ptr[f]))
        return o, out

    @staticmethod
    def _lam_rows(lam):
        """(lam as C-contiguous float64 [n_cw][n_slots], whether it was one codeword [n_slots])"""
        lam = np.asarray(lam, dtype=np.float64)
        return np.ascontiguousarray(lam.reshape(-1, lam.shape[-1])), lam.ndim == 1

    # -- BICM rate from the LLRs (DSCE_HAS_SOFT_RUN) --------------------------------
    def soft_shapes(self, sid):
        """Shapes of dsce_run_soft's arrays for scheme sid."""
        d = self.scheme_dims(sid)
        return dict(loss_est=(d.n_snr, d.n_iter + 1, 2), loss_perf0=(d.n_snr, 2))

    def run_soft(self, sid, seed, first_rep, n_rep, method="exact", out=None, branch="mmse"):
        """Information loss of the LLRs that export_llr would return for realisations
        [first_rep, first_rep + n_rep) of scheme sid, summed on the GPU
        (dsce_run_soft): dict of float64 arrays loss_est [n_snr][S][2] (MMSE branch,
        per stage; last axis 0 = all data symbols, 1 = the considered ones) and
        loss_perf0 [n_snr][2] (perfect-CSI one-tap receiver), in bits, summed over
        the realisations, the data symbols and their m bits (see
        dsce.modulation.bicm_info_loss).  The sums are ADDED into the arrays of
        `out` (a dict with either or both keys, C-contiguous float64; only the
        given ones are computed) and `out` is returned; without it both are
        computed from zero.  bicm_rate turns a sum into a rate.  branch 'perfect'
        (DSCE_LLR_PERFECT): loss_est receives the sums of the perfect-CSI branch at
        every stage, and loss_perf0 (its stage 0) may not be given."""
        o, out = self._acc_out(SoftOut, self.soft_shapes(sid), np.float64, out,
                               ("loss_est", "loss_perf0") if branch == "mmse" else ("loss_est",), "soft")
        self._chk(self.lib.dsce_run_soft(self.h, int(sid), int(seed), int(first_rep), int(n_rep),
                                         self._llr_flag(method) | self._branch_flag(branch), C.byref(o)),
                  "dsce_run_soft")
        return out

    def bicm_rate(self, sid, loss, n_rep):
        """I = m - loss / (n_rep ND_edge) bits per data symbol for sums `loss` of
        run_soft over n_rep realisations (last axis: the edge classes of
        bits_per_rep).  Exact LLRs: the BICM mutual-information estimate; max-log:
        the mismatched-decoder rate at scaling 1, a lower bound that may be
        negative."""
        m = self.llr_info(sid)["m"]
        nd = self.bits_per_rep(sid).astype(np.float64) / m
        return m - np.asarray(loss, dtype=np.float64) / (float(n_rep) * nd)

    # -- measured demapper noise (DSCE_HAS_LLR_SCALE) ---------------------------------
    def calib_shapes(self, sid):
        """Shapes of dsce_run_calib's arrays, and of the scale tables, for scheme sid."""
        d = self.scheme_dims(sid)
        return dict(ratio_est=(d.n_snr, d.n_iter + 1, d.n_data), ratio_perf0=(d.n_snr, d.n_data))

    def run_calib(self, sid, seed, first_rep, n_rep, out=None, branch="mmse"):
        """Demapper noise ratio of realisations [first_rep, first_rep + n_rep) of
        scheme sid, summed on the GPU (dsce_run_calib): dict of float64 arrays
        ratio_est [n_snr][S][ND] (MMSE branch, per stage and data symbol) and
        ratio_perf0 [n_snr][ND] (perfect-CSI one-tap receiver): the sums over the
        realisations of c |x_est - s_tx|^2 / pn_eff with the unscaled AWGN pn_eff
        (dsce.modulation.demapper_noise_ratio); rho = ratio / n_rep is what
        set_llr_scale takes.  The sums are ADDED into the arrays of `out` (a dict
        with either or both keys, C-contiguous float64; only the given ones are
        computed) and `out` is returned; without it both are computed from zero.
        branch 'perfect' (DSCE_LLR_PERFECT): ratio_est is the perfect-CSI branch's at
        every stage (rho for set_llr_scale_perf), and ratio_perf0 may not be given."""
        o, out = self._acc_out(CalibOut, self.calib_shapes(sid), np.float64, out,
                               ("ratio_est", "ratio_perf0") if branch == "mmse" else ("ratio_est",), "calibration")
        self._chk(self.lib.dsce_run_calib(self.h, int(sid), int(seed), int(first_rep), int(n_rep),
                                          self._branch_flag(branch), C.byref(o)), "dsce_run_calib")
        return out

    def set_llr_scale(self, sid, g_est=None, g_perf0=None):
        """Install the scale tables of scheme sid (dsce_set_llr_scale): g_est
        [n_snr][S][ND] multiplies pn_eff in export_llr and in run_soft's loss_est,
        g_perf0 [n_snr][ND] in run_soft's loss_perf0; None removes a table.  Every
        entry finite and > 0.  set_snr drops the tables."""
        shapes = self.calib_shapes(sid)
        ptr = []
        for g, f in ((g_est, "ratio_est"), (g_perf0, "ratio_perf0")):
            if g is None:
                ptr.append(None)
                continue
            g = np.ascontiguousarray(g, dtype=np.float64)
            if g.shape != shapes[f]:
                raise ValueError("scale table must have shape %s" % (shapes[f],))
            ptr.append(g)
        self._chk(self.lib.dsce_set_llr_scale(self.h, int(sid), *(None if g is None else _dptr(g) for g in ptr)),
                  "dsce_set_llr_scale")

    def llr_scale(self, sid):
        """dict(g_est, g_perf0, set) of scheme sid (dsce_get_llr_scale): the installed
        tables (ones where none is installed) and set = (bool, bool)."""
        shapes = self.calib_shapes(sid)
        g_est, g_perf0 = np.zeros(shapes["ratio_est"]), np.zeros(shapes["ratio_perf0"])
        set2 = (C.c_int32 * 2)()
        self._chk(self.lib.dsce_get_llr_scale(self.h, int(sid), _dptr(g_est), _dptr(g_perf0), set2),
                  "dsce_get_llr_scale")
        return dict(g_est=g_est, g_perf0=g_perf0, set=(bool(set2[0]), bool(set2[1])))

    def set_llr_scale_perf(self, sid, g_perf=None):
        """Install the scale table of the branch='perfect' calls of scheme sid
        (dsce_set_llr_scale_perf): g_perf [n_snr][S][ND] multiplies pn_eff in the
        flagged export_llr and run_soft; None removes it.  Every entry finite and
        > 0.  set_snr drops the table; the unflagged calls never read it."""
        if g_perf is not None:
            g_perf = np.ascontiguousarray(g_perf, dtype=np.float64)
            shape = self.calib_shapes(sid)["ratio_est"]
            if g_perf.shape != shape:
                raise ValueError("scale table must have shape %s" % (shape,))
        self._chk(self.lib.dsce_set_llr_scale_perf(self.h, int(sid), None if g_perf is None else _dptr(g_perf)),
                  "dsce_set_llr_scale_perf")

    def llr_scale_perf(self, sid):
        """dict(g_perf, set) of scheme sid (dsce_get_llr_scale_perf): the installed
        table (ones where none is installed) and set = bool."""
        g_perf = np.zeros(self.calib_shapes(sid)["ratio_est"])
        set1 = (C.c_int32 * 1)()
        self._chk(self.lib.dsce_get_llr_scale_perf(self.h, int(sid), _dptr(g_perf), set1), "dsce_get_llr_scale_perf")
        return dict(g_perf=g_perf, set=bool(set1[0]))

    # -- coded BER from a K = 7 Viterbi decoder (DSCE_HAS_CODED_RUN) -------------------
    @staticmethod
    def _code_desc(code):
        """(CodeDesc, the int32 table it points to) of a dsce.coding.Code"""
        src = np.ascontiguousarray(code.src, dtype=np.int32)
        if src.ndim != 2 or src.shape[1] != 2:
            raise ValueError("code.src must be [n_steps][2]")
        return CodeDesc(int(src.shape[0]), int(bool(code.terminated)), src.ctypes.data_as(C.POINTER(C.c_int32))), src

    def viterbi(self, lam, code):
        """The engine's decoder on caller-supplied lam [n_cw][n_slots] (or [n_slots];
        positive = the bit is 1) under the table of `code` (dsce.coding.make_code):
        uint8 [n_cw][n_steps] decoded inputs (dsce_viterbi), equal to the bit to
        dsce.coding.viterbi_decode.  Needs only the context."""
        lam, single = self._lam_rows(lam)
        desc, src = self._code_desc(code)
        out = np.zeros((lam.shape[0], src.shape[0]), dtype=np.uint8)
        self._chk(self.lib.dsce_viterbi(self.h, C.byref(desc), lam.shape[1], _dptr(lam), lam.shape[0],
                                        out.ctypes.data_as(C.POINTER(C.c_uint8))), "dsce_viterbi")
        return out[0] if single else out

    def coded_shapes(self, sid):
        """Shapes of dsce_run_coded's arrays for scheme sid."""
        d = self.scheme_dims(sid)
        return dict(bit_err=(d.n_snr, d.n_iter + 1), frame_err=(d.n_snr, d.n_iter + 1))

    def run_coded(self, sid, seed, first_rep, n_rep, code, method="exact", out=None, branch="mmse"):
        """Decoded-error counts of the K = 7 convolutional code of `code`
        (dsce.coding.make_code(ND m, rate)) over the LLRs that export_llr would
        return for realisations [first_rep, first_rep + n_rep) of scheme sid, one
        codeword per realisation, SNR point and stage, decoded on the GPU
        (dsce_run_coded): dict of int64 arrays bit_err and frame_err [n_snr][S].
        The all-zero information word is simulated under the BITS stream as the
        scrambler, which is exact for a linear code (include/dsce.h).  The counts
        are ADDED into the arrays of `out` (a dict with either or both keys,
        C-contiguous int64; only the given ones are computed) and `out` is
        returned; without it both are computed from zero.  BER = bit_err / (n_rep
        code.n_info), FER = frame_err / n_rep.  branch 'perfect'
        (DSCE_LLR_PERFECT): the LLRs of the perfect-CSI branch."""
        shapes = self.coded_shapes(sid)
        o, out = self._acc_out(CodedOut, shapes, np.int64, out, tuple(shapes), "coded")
        desc, src = self._code_desc(code)
        self._chk(self.lib.dsce_run_coded(self.h, int(sid), int(seed), int(first_rep), int(n_rep),
                                          self._llr_flag(method) | self._branch_flag(branch), C.byref(desc),
                                          C.byref(o)), "dsce_run_coded")
        return out

    # -- coded BER from a normalised min-sum LDPC decoder (DSCE_HAS_LDPC_RUN) ---------
    @staticmethod
    def _ldpc_desc(code):
        """(LdpcDesc, the int32 arrays it points to) of a dsce.coding.LdpcCode"""
        keep = tuple(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32)
                     for a in (code.row_ptr, code.col, code.slot))
        if keep[0].size != int(code.n_checks) + 1 or keep[2].size != int(code.n_vars):
            raise ValueError("row_ptr must be [n_checks + 1] and slot [n_vars]")
        if keep[0].size and keep[1].size != keep[0][-1]:
            raise ValueError("col must have row_ptr[n_checks] entries")
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
        return LdpcDesc(int(code.n_vars), int(code.n_checks), ptr[0], ptr[1], ptr[2], int(code.n_info),
                        int(code.max_iter), float(code.alpha), int(code.early_stop)), keep

    @staticmethod
    def _ldpc_layers(layers, code):
        """(LdpcLayers, the int32 arrays it points to) of (layer_ptr, layer_check) (dsce.coding.make_layers)"""
        keep = tuple(np.ascontiguousarray(np.asarray(a).reshape(-1), dtype=np.int32) for a in layers)
        if len(keep) != 2 or keep[0].size < 1 or keep[1].size != int(code.n_checks):
            raise ValueError("layers must be (layer_ptr [n_layers + 1], layer_check [n_checks])")
        ptr = [a.ctypes.data_as(C.POINTER(C.c_int32)) for a in keep]
        return LdpcLayers(keep[0].size - 1, ptr[0], ptr[1]), keep

    @staticmethod
    def _ldpc_fixed(fx):
        """LdpcFixedDesc of a dsce.coding.LdpcFixed"""
        return LdpcFixedDesc(float(fx.scale), int(fx.q_ch), int(fx.q_msg), int(fx.q_app), int(fx.alpha_num),
                             int(fx.alpha_shift), int(fx.beta))

    def ldpc(self, lam, code, layers=None, fixed=None):
        """The engine's min-sum decoder on caller-supplied lam [n_cw][n_slots] (or
        [n_slots]; positive = the bit is 1) under `code` (dsce.coding.make_ldpc):
        (x uint8 [n_cw][n_vars], it int32 [n_cw]), the decided bits and the
        iterations performed (dsce_ldpc), equal to the bit to
        dsce.coding.ldpc_decode.  With layers = (layer_ptr, layer_check)
        (dsce.coding.make_layers) the layered schedule (dsce_ldpc_layered), equal to
        the bit to dsce.coding.ldpc_decode_layered.  With fixed = an LdpcFixed
        (dsce.coding.make_fixed) the fixed-point decoder (dsce_ldpc_fixed), equal to
        dsce.coding.ldpc_decode_fixed, and a third result: app int16 [n_cw][n_vars],
        the final a-posteriori sums.  Needs only the context."""
        if fixed is not None and layers is not None:
            raise ValueError("fixed and layers exclude each other: the fixed-point decoder has the flooding schedule")
        lam, single = self._lam_rows(lam)
        desc, keep = self._ldpc_desc(code)
        x = np.zeros((lam.shape[0], int(code.n_vars)), dtype=np.uint8)
        it = np.zeros(lam.shape[0], dtype=np.int32)
        xp, ip = x.ctypes.data_as(C.POINTER(C.c_uint8)), it.ctypes.data_as(C.POINTER(C.c_int32))
        if fixed is not None:
            app = np.zeros(x.shape, dtype=np.int16)
            fd = self._ldpc_fixed(fixed)
            self._chk(self.lib.dsce_ldpc_fixed(self.h, C.byref(desc), C.byref(fd), lam.shape[1], _dptr(lam), lam.shape[0],
                                               xp, ip, app.ctypes.data_as(C.POINTER(C.c_int16))), "dsce_ldpc_fixed")
            return (x[0], it[0], app[0]) if single else (x, it, app)
        if layers is None:
            self._chk(self.lib.dsce_ldpc(self.h, C.byref(desc), lam.shape[1], _dptr(lam), lam.shape[0], xp, ip),
                      "dsce_ldpc")
        else:
            ly, keep_l = self._ldpc_layers(layers, code)
            self._chk(self.lib.dsce_ldpc_layered(self.h, C.byref(desc), C.byref(ly), lam.shape[1], _dptr(lam),
                                                 lam.shape[0], xp, ip), "dsce_ldpc_layered")
        return (x[0], it[0]) if single else (x, it)

    def ldpc_shapes(self, sid):
        """Shapes of dsce_run_ldpc's arrays for scheme sid."""
        d = self.scheme_dims(sid)
        return {f: (d.n_snr, d.n_iter + 1) for f in ("bit_err", "frame_err", "iter_sum")}

    def run_ldpc(self, sid, seed, first_rep, n_rep, code, method="exact", out=None, branch="mmse", layers=None,
                 fixed=None, codeword=None):
        """Decoded-error counts of the LDPC code `code` (dsce.coding.make_ldpc(ND m,
        rate)) over the LLRs that export_llr would return for realisations
        [first_rep, first_rep + n_rep) of scheme sid, one codeword per realisation,
        SNR point and stage, decoded on the GPU by normalised min-sum
        (dsce_run_ldpc): dict of int64 arrays bit_err, frame_err and iter_sum
        [n_snr][S].  The all-zero codeword is simulated under the BITS stream as
        the scrambler, which is exact for this decoder (include/dsce.h).  The
        counts are ADDED into the arrays of `out` (a dict with any of the keys,
        C-contiguous int64; only the given ones are computed) and `out` is
        returned; without it all are computed from zero.  BER = bit_err / (n_rep
        code.n_info), FER = frame_err / n_rep, mean iterations = iter_sum / n_rep.
        branch 'perfect' (DSCE_LLR_PERFECT): the LLRs of the perfect-CSI branch.
        layers = (layer_ptr, layer_check) (dsce.coding.make_layers): the layered
        schedule over that partition of the checks (dsce_run_ldpc_layered).
        fixed = an LdpcFixed (dsce.coding.make_fixed): the fixed-point decoder
        (dsce_run_ldpc_fixed), with codeword = a word of the code (uint8 [n_vars],
        dsce.coding.ldpc_encode) transmitted in place of the all-zero word, which
        in integers is optimistic at ties (include/dsce.h); bit_err then counts the
        decided information bits that differ from it."""
        if fixed is not None and layers is not None:
            raise ValueError("fixed and layers exclude each other: the fixed-point decoder has the flooding schedule")
        if codeword is not None and fixed is None:
            raise ValueError("codeword needs fixed: the fp64 decoders simulate the all-zero word, which is exact for them")
        shapes = self.ldpc_shapes(sid)
        o, out = self._acc_out(LdpcOut, shapes, np.int64, out, tuple(shapes), "ldpc")
        desc, keep = self._ldpc_desc(code)
        flags = self._llr_flag(method) | self._branch_flag(branch)
        if fixed is not None:
            fd = self._ldpc_fixed(fixed)
            word = None
            if codeword is not None:
                word = np.ascontiguousarray(np.asarray(codeword).reshape(-1), dtype=np.uint8)
                if word.size != int(code.n_vars):
                    raise ValueError("codeword must have n_vars entries")
            wp = None if word is None else word.ctypes.data_as(C.POINTER(C.c_uint8))
            self._chk(self.lib.dsce_run_ldpc_fixed(self.h, int(sid), int(seed), int(first_rep), int(n_rep), flags,
                                                   C.byref(desc), C.byref(fd), wp, C.byref(o)), "dsce_run_ldpc_fixed")
            return out
        if layers is None:
            self._chk(self.lib.dsce_run_ldpc(self.h, int(sid), int(seed), int(first_rep), int(n_rep), flags,
                                             C.byref(desc), C.byref(o)), "dsce_run_ldpc")
        else:
            ly, keep_l = self._ldpc_layers(layers, code)
            self._chk(self.lib.dsce_run_ldpc_layered(self.h, int(sid), int(seed), int(first_rep), int(n_rep), flags,
                                                     C.byref(desc), C.byref(ly), C.byref(o)), "dsce_run_ldpc_layered")
        return out

    # -- engine state ------------------------------------------------------------
    def scheme_dims(self, sid):
        d = Dims()
        self._chk(self.lib.dsce_scheme_dims(self.h, int(sid), C.byref(d)), "dsce_scheme_dims")
        return d

    def path_info(self, sid):
        """Names of the kernel paths the scheme's last run / trace went through."""
        f = C.c_uint32()
        self._chk(self.lib.dsce_path_info(self.h, int(sid), C.byref(f)), "dsce_path_info")
        return {k for k, bit in PATH_BITS.items() if f.value & bit}

    def jakes_info(self):
        """The Jakes kernel of the last run / trace / channel_impulse_response
        (dsce_jakes_info): dict with kernel ('static' | 'discrete' | 'full' |
        'win_rec' | 'win_mom' | 'win_grp'; 'none' before the first), and for
        'win_grp' grp2 (k_jakes_grp2 instead of k_jakes_grp), ngrp, lg, mt (the
        template instance <mt, lg>); chunks = window chunks formed (0: all samples)."""
        out = (C.c_int32 * 6)()
        self._chk(self.lib.dsce_jakes_info(self.h, out), "dsce_jakes_info")
        return dict(kernel=JAKES_KERNELS.get(out[0], str(out[0])), grp2=bool(out[1]), ngrp=out[2], lg=out[3],
                    mt=out[4], chunks=out[5])

    def set_option(self, name, value):
        self._chk(self.lib.dsce_set_option(self.h, name.encode(), int(value)), "dsce_set_option(%s)" % name)

    def get_option(self, name):
        v = C.c_int64()
        self._chk(self.lib.dsce_get_option(self.h, name.encode(), C.byref(v)), "dsce_get_option(%s)" % name)
        return v.value

    def mmse_onetap(self, sid, snr_index, hp_ls, variant=0):
        """h_hat = diag(sum_p W_p hP_p) for LS vectors hp_ls (NP,) or (NP, n)."""
        sc = self.schemes[sid]
        hp = np.asarray(hp_ls, dtype=np.complex128)
        one = hp.ndim == 1
        hp = np.ascontiguousarray(hp.reshape(sc.n_pilots, -1).T)      # n x NP rows = column-major NP x n
        n = hp.shape[0]
        out = np.zeros(2 * sc.LK * n)
        self._chk(self.lib.dsce_mmse_onetap(self.h, int(sid), int(snr_index), int(variant),
                                            hp.ctypes.data_as(C.POINTER(C.c_double)), n, _dptr(out)),
                  "dsce_mmse_onetap")
        h = out.view(np.complex128).reshape(n, sc.LK).T
        return h[:, 0] if one else h

    # -- channel-estimation MSE (build-defined) ---------------------------------
    def enable_mse(self, on=True):
        """Start (and reset) the MSE sums of dsce_run (dsce_enable_mse)."""
        self._chk(self.lib.dsce_enable_mse(self.h, int(bool(on))), "dsce_enable_mse")

    def mse(self):
        """(err [scheme][snr][stage] = sum |h_hat - h|^2, pow [scheme][snr] = sum |h|^2)
        since enable_mse(); NMSE = err / pow[..., None]."""
        ns = len(self.schemes)
        err = np.zeros((ns, self.nsnr, 1 + self.niter))
        pw = np.zeros((ns, self.nsnr))
        self._chk(self.lib.dsce_get_mse(self.h, _dptr(err), _dptr(pw)), "dsce_get_mse")
        return err, pw

    def group_info(self):
        """(devices, reduce) of the context (dsce_group_info): the members' HIP
        devices and how run() sums them ('none' | 'rccl' | 'host')."""
        n = C.c_int32()
        self._chk(self.lib.dsce_group_info(self.h, C.byref(n), None, None), "dsce_group_info")
        devs = np.zeros(n.value, dtype=np.int32)
        red = C.c_int32()
        self._chk(self.lib.dsce_group_info(self.h, None, devs.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(red)),
                  "dsce_group_info")
        return [int(d) for d in devs], REDUCE.get(red.value, str(red.value))

    # -- measurement -----------------------------------------------------------
    def enable_timing(self, on=True):
        self._chk(self.lib.dsce_enable_timing(self.h, int(bool(on))), "dsce_enable_timing")

    def kernel_time(self, name):
        n = C.c_int64()
        ms = C.c_double()
        self._chk(self.lib.dsce_kernel_time(self.h, name.encode(), C.byref(n), C.byref(ms)), "dsce_kernel_time")
        return n.value, ms.value

    def fp64_mfma_peak(self):
        """Measured FP64 matrix-core peak of this GPU, TFLOP/s (dsce_fp64_mfma_peak)."""
        t = C.c_double()
        self._chk(self.lib.dsce_fp64_mfma_peak(self.h, C.byref(t)), "dsce_fp64_mfma_peak")
        return t.value

    def kernel_work(self, name):
        """(flops, bytes) per realisation of timed kernel group `name` (dsce_kernel_work;
        0 = not modelled for the path that ran)."""
        f = C.c_double()
        b = C.c_double()
        self._chk(self.lib.dsce_kernel_work(self.h, name.encode(), C.byref(f), C.byref(b)), "dsce_kernel_work")
        return f.value, b.value

    def structured_check(self, sid):
        """build_mic's guard of the structured MMSE IC (dsce_structured_check): dict with
        ratio (kept iff <= 1: the worst slice's deviation over its rounding bar
        min(1e-9, max(1e-11, 4e-16 kappa(R))) max|W|), dev (max |Q' H_hat G - W_thr|),
        wmax (max |W|), rtol (the largest per-slice bar), and the low-rank tap
        operator's fit residual lr_resid (relative), lr (built and kept: eligible; a
        run uses it with option mic_lr = 1, see path_info's mic_lr) and lr_ratio
        (capped bar min(1e-9, max(1e-13, 4e-16 kappa(R))))."""
        out = (C.c_double * 7)()
        self._chk(self.lib.dsce_structured_check(self.h, int(sid), out), "dsce_structured_check")
        return dict(ratio=out[0], dev=out[1], wmax=out[2], rtol=out[3], lr_resid=out[4], lr=bool(out[5]),
                    lr_ratio=out[6])

    def work_model(self, sid):
        cm = C.c_double()
        wb = C.c_double()
        self._chk(self.lib.dsce_work_model(self.h, int(sid), C.byref(cm), C.byref(wb)), "dsce_work_model")
        return cm.value, wb.value


# The bulk exports, one description each: the entry point, its ctypes struct, its
# fields in the struct's order, each field's kind ("complex": complex128, or
# complex64 with DSCE_EXPORT_F32; "real": float64 / float32; "int32"), what the
# fields are called in a message, and shapes(engine, sid, n_rep).
_ExportKind = collections.namedtuple("_ExportKind", "entry struct fields kinds noun shapes")
_EXPORTS = {
    "export": _ExportKind("dsce_export", ExportOut, EXPORT_FIELDS,
                          dict(zip(EXPORT_FIELDS, ("complex",) * 5 + ("int32",))), "export", Engine.export_shapes),
    "stages": _ExportKind("dsce_export_stages", ExportStagesOut, STAGE_FIELDS,
                          dict(zip(STAGE_FIELDS, ("complex",) * 3 + ("int32",) * 2)), "stage export",
                          Engine.export_stages_shapes),
    "llr": _ExportKind("dsce_export_llr", ExportLlrOut, LLR_FIELDS,
                       dict(zip(LLR_FIELDS, ("complex", "real", "real"))), "LLR export", Engine.export_llr_shapes),
}


class _HostArrays:
    """NumPy arrays for Engine._bulk_export, complex fields of `dtype`."""

    def __init__(self, dtype):
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.complex128), np.dtype(np.complex64)):
            raise ValueError("export dtype must be complex128 or complex64")
        f32 = dt == np.dtype(np.complex64)
        self.flags = EXPORT_F32 if f32 else 0
        self.types = {"complex": dt, "real": np.dtype(np.float32 if f32 else np.float64), "int32": np.int32}

    def empty(self, shape, kind):
        return np.zeros(shape, dtype=self.types[kind])

    def ready(self):
        pass

    @staticmethod
    def address(a):
        return a.ctypes.data


class _TorchArrays:
    """torch tensors on the context's GPU for Engine._bulk_export (`what`: the
    calling method, for messages), written in place (DSCE_EXPORT_DEVICE)."""

    def __init__(self, eng, what, dtype, device):
        import torch
        dtype = torch.complex128 if dtype is None else dtype
        if dtype not in (torch.complex128, torch.complex64):
            raise ValueError("%s dtype must be torch.complex128 or torch.complex64" % what)
        if not torch.cuda.is_available():
            raise DsceError("%s: torch sees no HIP device in this process; import torch before the "
                            "first dsce.engine.Engine is created so that both use one HIP runtime" % what)
        if device is None:
            device = eng.group_info()[0][0]
        f32 = dtype == torch.complex64
        self.torch = torch
        self.dev = "cuda:%d" % int(device)
        self.flags = EXPORT_DEVICE | (EXPORT_F32 if f32 else 0)
        self.types = {"complex": dtype, "real": torch.float32 if f32 else torch.float64, "int32": torch.int32}

    def empty(self, shape, kind):
        return self.torch.empty(shape, dtype=self.types[kind], device=self.dev)

    def ready(self):
        # the allocations (and any work torch queued on them) precede the engine's stream
        self.torch.cuda.current_stream(self.dev).synchronize()

    @staticmethod
    def address(t):
        return t.data_ptr()


def gpu_tx(device=0):
    """Producer of (G, Q) for build_setup(tx=...): dsce_tx_matrices on `device`
    (row f1, OFDM.m:184-218 / FBMC.m:318-354 in closed form per element)."""
    def produce(mod):
        eng = Engine(device)
        try:
            return eng.tx_matrices(mod)
        finally:
            eng.close()
    return produce


def build_engine(setup, schemes=None, device=0, zero_threshold=None, batch=None, options=None, mmse=True):
    """Engine configured like the script: channel, SNR list, schemes, MMSE setup.
    ``options``: dsce_set_option name -> value, applied before the MMSE build.
    ``mmse=False`` leaves dsce_build_mmse out (enough for the probes and for
    export() without h_est)."""
    eng = Engine(device)
    for k, v in (options or {}).items():
        eng.set_option(k, v)
    eng.set_channel(setup.channel)
    eng.set_snr(setup.pn_time, setup.n_iter)
    names = list(setup.schemes) if schemes is None else list(schemes)
    for n in names:
        eng.add_scheme(setup.schemes[n])
    if mmse:
        eng.build_mmse(setup.zero_threshold if zero_threshold is None else zero_threshold)
    if batch:
        eng.set_batch(batch)
    return eng
