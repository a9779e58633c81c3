"""Every launcher's dispatch once, for a (kernel name, calls) table under
rocprofv3 --kernel-trace --stats: the three configs, the doubly-flat setup, one
FBMC scheme alone, one export_stages and one run_soft on the perfect-CSI
branch, each at 64 realisations, batch 64 and two SNR points.  Two builds
launched the same kernels when their tables are equal (tools/launch_table.py).
usage: launch_probe.py"""
import os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path[:0] = [R, R + '/channel-estimation_amd']
from dsce.configs import _CONFIGS, build_doubly_flat_setup, build_setup
from dsce.doubly_flat import DoublyFlatSim
from dsce.engine import build_engine

SEED, N, SNR = 0x5EED0002, 64, [15.0, 35.0]
ALL = ("fbmc_aux", "fbmc_cod", "ofdm")
# the paper config with the scheme the suite runs it with (tests/test_gpu_paper.py)
for name, schemes in [(n, ("fbmc_aux",) if n == "paper" else ALL) for n in sorted(_CONFIGS)] + [("default", ("fbmc_cod",))]:
    eng = build_engine(build_setup(name, schemes=schemes, snr_db=SNR), batch=N)
    eng.run(SEED, 0, N)
    print(name, schemes, eng.jakes_info(), [sorted(eng.path_info(i)) for i in range(len(schemes))], flush=True)
    eng.close()
sim = DoublyFlatSim(build_doubly_flat_setup(snr_db=SNR), batch=N)
sim.run(SEED, 0, N)
sim.close()
eng = build_engine(build_setup("default", schemes=("ofdm",), snr_db=SNR), batch=N)
eng.export_stages(0, SEED, 0, N)
eng.run_soft(0, SEED, 0, N, branch="perfect")
eng.close()
print('ok')
