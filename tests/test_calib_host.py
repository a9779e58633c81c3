"""CPU: the host side of the measured demapper noise (dsce_run_calib /
dsce_set_llr_scale / dsce_get_llr_scale, DSCE_HAS_LLR_SCALE) — the header's
declarations against the ctypes binding, the NumPy twin
dsce.modulation.demapper_noise_ratio against its closed form, and the command
line's --calibrate.  No GPU call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import harness

HDR = os.path.join(harness.ROOT, "include", "dsce.h")


def test_header_declares_calib_and_binding_matches(tmp_path):
    from dsce import engine
    txt = open(HDR).read()
    for fn in ("dsce_run_calib", "dsce_set_llr_scale", "dsce_get_llr_scale"):
        assert re.search(r"^int\s+%s\s*\(" % fn, txt, re.M), fn
        assert fn in engine.EXPORTED
    assert re.search(r"^#define DSCE_HAS_LLR_SCALE\s+1\b", txt, re.M)
    assert re.search(r"#define DSCE_ABI_VERSION\s+10\b", txt) and engine.ABI_VERSION == 10
    body = re.search(r"typedef struct \{([^}]*)\} dsce_calib_out;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"double\s*\*\s*(\w+)\s*;", body)
    assert fields == [f for f, _ in engine.CalibOut._fields_] == ["ratio_est", "ratio_perf0"]
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   '#if !DSCE_HAS_LLR_SCALE || DSCE_ABI_VERSION != 10\n#error "calibration macros"\n#endif\n'
                   'int (*run)(dsce_ctx*, int32_t, uint64_t, uint64_t, uint64_t, uint32_t, const dsce_calib_out*)'
                   ' = dsce_run_calib;\n'
                   'int (*set)(dsce_ctx*, int32_t, const double*, const double*) = dsce_set_llr_scale;\n'
                   'int (*get)(dsce_ctx*, int32_t, double*, double*, int32_t*) = dsce_get_llr_scale;\n')
    obj = tmp_path / "c.o"
    # the prototypes are checked by compiling these assignments (not linked); the layout by a program
    subprocess.run(["gcc", "-Werror", "-I", os.path.dirname(HDR), "-c", str(src), "-o", str(obj)], check=True)
    lay = tmp_path / "lay.c"
    lay.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\n'
                   'int main(){printf("%zu", sizeof(dsce_calib_out));\n'
                   + "".join('printf(" %%zu", offsetof(dsce_calib_out, %s));\n' % f for f in fields)
                   + "return 0;}\n")
    exe = tmp_path / "lay"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(lay), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    assert c == [ctypes.sizeof(engine.CalibOut)] + [getattr(engine.CalibOut, f).offset for f in fields]
    # the binding's argument lists, when the library is built
    if os.path.exists(engine.LIB_PATH):
        lib = engine.load_library()
        dp, vp = ctypes.POINTER(ctypes.c_double), ctypes.c_void_p
        assert lib.dsce_run_calib.argtypes == [vp, ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64,
                                               ctypes.c_uint32, ctypes.POINTER(engine.CalibOut)]
        assert lib.dsce_set_llr_scale.argtypes == [vp, ctypes.c_int32, dp, dp]
        assert lib.dsce_get_llr_scale.argtypes == [vp, ctypes.c_int32, dp, dp, ctypes.POINTER(ctypes.c_int32)]


@pytest.mark.parametrize("real_detect,bar", [(False, 0.012), (True, 0.016)], ids=["complex", "real"])
def test_noise_ratio_closed_form(real_detect, bar):
    """x = s + sqrt(g0 pn / 2) (n1 + j n2) over 200 000 seeded samples, random
    symbols, pn in 10^[-4, 0]: the mean ratio is g0 within 1.2 % (five standard
    errors of an exponential variate's mean: 5 / sqrt(2e5) = 1.12 %).  Real
    detection: one normal, c = 2, so the ratio is g0 chi^2_1 with standard
    deviation sqrt(2) g0: 5 sqrt(2) / sqrt(2e5) = 1.58 %, bar 1.6 %."""
    from dsce.modulation import SignalConstellation, demapper_noise_ratio
    n, g0 = 200000, 3.7
    rng = np.random.default_rng(2024)
    c = SignalConstellation(16, "PAM") if real_detect else SignalConstellation(256, "QAM")
    symbols = np.asarray(c.SymbolMapping).reshape(-1)
    sym = rng.integers(0, symbols.size, n)
    pn = 10.0 ** rng.uniform(-4, 0, n)
    n1, n2 = rng.standard_normal(n), rng.standard_normal(n)
    if real_detect:
        x = symbols[sym].real + np.sqrt(g0 * pn / 2) * n1 + 0j
    else:
        x = symbols[sym] + np.sqrt(g0 * pn / 2) * (n1 + 1j * n2)
    r = demapper_noise_ratio(x, pn, sym, symbols, real_detect)
    assert r.shape == (n,) and (r >= 0).all()
    print("noise ratio closed form: mean / g0 - 1 = %.3e (bar %.3e)" % (r.mean() / g0 - 1, bar))
    assert abs(r.mean() / g0 - 1) <= bar
    # any leading shape, broadcasting sym against [snr][stage] axes
    x4 = np.broadcast_to(x[:24].reshape(2, 1, 1, 12), (2, 3, 5, 12))
    p4 = np.broadcast_to(pn[:24].reshape(2, 1, 1, 12), (2, 3, 5, 12))
    r4 = demapper_noise_ratio(x4, p4, sym[:24].reshape(2, 1, 1, 12), symbols, real_detect)
    assert r4.shape == (2, 3, 5, 12) and np.array_equal(r4[:, 1, 2].reshape(-1), r[:24])


def test_calibrate_needs_rate():
    from dsce import simulate
    with pytest.raises(SystemExit) as e:
        simulate.main(["--config", "default", "--schemes", "ofdm", "--reps", "8", "--calibrate"])
    assert "--calibrate needs --rate" in str(e.value)
