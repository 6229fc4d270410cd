"""The kernel-unit rule of the C ABI (csrc/units.h) on the CPU, through the test-only host build: which engine, Decima,
greedy-Decima and priority unit a launch on a layout runs, and the Decima unit's waves per workgroup. The rule reads
only num_executors, job_cap, stage_cap, the residency and the SSIM_GENERIC switch, so the layouts are set directly.
The table is written out row by row, not computed from the rule; the gfx950 library's names for real layouts are
asserted by the `-m gpu` tests."""

import ctypes as ct
import os
import re

import pytest

from hostsim.driver import REPO, lib
from spark_sched_sim._abi import SsimLayout

LDS, HBM = 1, 0
HELP = "kDpHelpWaves"
# (residency, (N, J, stage cap), generic) -> engine, decima, greedy, waves; stage cap None = any
TABLE = [
    (LDS, (10, 50, 900), 0, "bench900", "dr_lds", "drg_lds", 1),
    (LDS, (10, 50, 900), 1, "bench900", "dr_lds", "drg_lds", 1),
    (LDS, (10, 50, 850), 0, "bench", "dr_lds", "drg_lds", 1),
    (LDS, (10, 50, 850), 1, "bench", "dr_lds", "drg_lds", 1),
    (LDS, (50, 200, None), 0, "lds", "dr_lds50", "drg_lds50", HELP),
    (LDS, (50, 200, None), 1, "lds", "dr_lds", "drg_lds", 1),
    (LDS, (20, 30, None), 0, "lds", "dr_lds", "drg_lds", 1),
    (LDS, (20, 30, None), 1, "lds", "dr_lds", "drg_lds", 1),
    (HBM, (100, 200, None), 0, "hbm_n100", "dr_hbm", "drg_hbm", 1),
    (HBM, (100, 200, None), 1, "hbm", "dr_hbm", "drg_hbm", 1),
    (HBM, (50, 200, None), 0, "hbm_n50", "dr_hbm50", "drg_hbm50", 1),
    (HBM, (50, 200, None), 1, "hbm", "dr_hbm", "drg_hbm", 1),
    (HBM, (10, 50, None), 0, "hbm_n10", "dr_hbm", "drg_hbm", 1),
    (HBM, (10, 50, None), 1, "hbm", "dr_hbm", "drg_hbm", 1),
    (HBM, (127, 50, None), 0, "hbm", "dr_hbm", "drg_hbm", 1),
    (HBM, (127, 50, None), 1, "hbm", "dr_hbm", "drg_hbm", 1),
]


def help_waves() -> int:
    """decima_policy.h kDpHelpWaves (a device header the host build cannot include)."""
    text = open(os.path.join(REPO, "gym-sparksched_amd", "csrc", "decima_policy.h")).read()
    return int(re.search(r"constexpr int kDpHelpWaves = (\d+);", text).group(1))


def unit_names(resident, N, J, S, generic):
    L = SsimLayout(num_executors=N, job_cap=J, stage_cap=S, lds_resident=resident)
    names = [ct.c_char_p() for _ in range(4)]
    waves = ct.c_int(-1)
    lib().hs_unit_names(ct.byref(L), resident, generic, *[ct.byref(n) for n in names], ct.byref(waves))
    return tuple(n.value.decode() for n in names) + (waves.value,)


@pytest.mark.parametrize("resident,shape,generic,engine,decima,greedy,waves", TABLE)
def test_unit_rule(resident, shape, generic, engine, decima, greedy, waves):
    N, J, S = shape
    for cap in ([S] if S is not None else [900, 850, 18 * J]):  # ("any": the synthetic set's 900, and two others)
        got = unit_names(resident, N, J, cap, generic)
        want = (engine, decima, greedy, "prio_lds" if resident else "prio_hbm", help_waves() if waves == HELP else 1)
        assert got == want, (resident, N, J, cap, generic)

