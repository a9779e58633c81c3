"""CPU: the C-ABI shared library loads and exports exactly the entry points
declared in include/dsce.h; the ctypes structures match the C layout.  No
compute calls (no GPU in this container)."""
import os
import re
import subprocess

import pytest

import harness

HDR = os.path.join(harness.ROOT, "include", "dsce.h")
LIB = os.path.join(harness.PKG, "dsce", "libdsce.so")


def declared():
    txt = open(HDR).read()
    return sorted(set(re.findall(r"^\s*(?:int|void|const char\*)\s+(dsce_\w+)\s*\(", txt, re.M)))


def test_header_and_binding_agree():
    from dsce import engine
    assert sorted(engine.EXPORTED) == declared()


def test_library_exports_every_declared_symbol():
    if not os.path.exists(LIB):
        pytest.skip("libdsce.so not built (run __graft_entry__.build())")
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    syms = set(re.findall(r"\bT (dsce_\w+)", out))
    missing = [s for s in declared() if s not in syms]
    assert not missing, missing
    from dsce import engine
    lib = engine.load_library()
    assert lib.dsce_abi_version() == engine.ABI_VERSION


def test_struct_layout_matches_c(tmp_path):
    import ctypes

    from dsce import engine
    src = tmp_path / "l.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "dsce.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu '
                   '%zu %zu %zu %zu\\n",'
                   'sizeof(dsce_channel_desc), sizeof(dsce_scheme_desc), offsetof(dsce_scheme_desc, kappa),'
                   'offsetof(dsce_scheme_desc, G), offsetof(dsce_scheme_desc, symbols), sizeof(dsce_tx_desc),'
                   'offsetof(dsce_tx_desc, norm), sizeof(dsce_dims), offsetof(dsce_dims, n_counters),'
                   'sizeof(dsce_trace), offsetof(dsce_trace, dec_perf));return 0;}\n')
    exe = tmp_path / "l"
    subprocess.run(["gcc", "-I", os.path.dirname(HDR), str(src), "-o", str(exe)], check=True)
    c = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    py = [ctypes.sizeof(engine.ChannelDesc), ctypes.sizeof(engine.SchemeDesc), engine.SchemeDesc.kappa.offset,
          engine.SchemeDesc.G.offset, engine.SchemeDesc.symbols.offset, ctypes.sizeof(engine.TxDesc),
          engine.TxDesc.norm.offset, ctypes.sizeof(engine.Dims), engine.Dims.n_counters.offset,
          ctypes.sizeof(engine.Trace), engine.Trace.dec_perf.offset]
    assert c == py


def test_no_cpu_fallback_without_gpu():
    """The product path fails loudly when no HIP device is usable."""
    if not os.path.exists(LIB):
        pytest.skip("libdsce.so not built")
    from dsce import engine
    n = engine.load_library()
    import ctypes
    cnt = ctypes.c_int(0)
    n.dsce_device_count(ctypes.byref(cnt))
    if cnt.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(engine.DsceError):
        engine.Engine(0)
    with pytest.raises(engine.DsceError):
        engine.Engine([0, 1])                    # dsce_create_multi (ABI 7) fails loudly too


def test_jakes_info_is_exported_and_rejects_null():
    """dsce_jakes_info (ABI 8): exported, bound, and a null context is a clean
    DSCE_EINVAL (no HIP call is made for it, so this needs no GPU)."""
    if not os.path.exists(LIB):
        pytest.skip("libdsce.so not built")
    import ctypes

    from dsce import engine
    assert "dsce_jakes_info" in engine.EXPORTED and engine.ABI_VERSION >= 8
    lib = engine.load_library()
    out = (ctypes.c_int32 * 6)()
    assert lib.dsce_jakes_info(None, out) == -1          # DSCE_EINVAL
    assert sorted(engine.JAKES_KERNELS) == list(range(7))
    txt = open(HDR).read()
    for v, name in engine.JAKES_KERNELS.items():
        assert re.search(r"#define DSCE_JAKES_%s\s+%d\b" % (name.upper(), v), txt), name


def test_library_links_rccl_and_roctx():
    """The in-library all-reduce (dsce_create_multi) and the host trace ranges
    (roctx) are linked dependencies of libdsce.so."""
    import subprocess
    if not os.path.exists(LIB):
        pytest.skip("libdsce.so not built")
    out = subprocess.run(["readelf", "-d", LIB], check=True, capture_output=True, text=True).stdout
    needed = [l.split("[")[1].rstrip("]") for l in out.splitlines() if "(NEEDED)" in l]
    assert any(n.startswith("librccl.so") for n in needed), needed
    assert any(n.startswith("librocprofiler-sdk-roctx.so") for n in needed), needed


def test_asan_driver_is_instrumented():
    """tools/asan/dsce_asan_driver (`make -f asan.mk`, tests/test_gpu_asan.py) carries
    a live host sanitizer: its --probe mode's one-past-the-end heap read is
    reported (no GPU needed)."""
    import subprocess
    b = os.path.join(harness.ROOT, "tools", "asan", "dsce_asan_driver")
    if not os.path.exists(b):
        pytest.skip("asan driver not built (make -C channel-estimation_amd -f asan.mk)")
    p = subprocess.run([b, "--probe"], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), capture_output=True,
                       text=True, timeout=60)
    assert p.returncode != 0 and "heap-buffer-overflow" in p.stderr, p.stderr[-2000:]
