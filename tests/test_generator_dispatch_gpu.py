"""Which kernels a whole-network generator entry launches (csrc/network.hip: plan_generator).

For every case of tests/generator_cases.py that runs on the GPU — image sizes from 16 x 16 to 224 x 224, both arithmetic modes, init_features 16 and 32, the three
entries, taps, each kernel switch and each chain count, every switch set and unset around the single call — one forward runs between profile_start() and
profile_stop(); the recorded launch names must equal EXPECTED.  EXPECTED was recorded by running this same table on the commit BEFORE the dispatch was rewritten around
plan_generator: the rewrite must launch what that commit launched, name by name.  The report of smirk_generator_plan, asked in the same process under the same
switches, must stand for the same names (the launch profiler keeps one chain, so a report with several chains is held to everything outside the section here and
to its single-chain sibling cases by tests/test_generator_dispatch_cpu.py)."""
import pytest

import generator_cases as GC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", GC.GPU_CASES)
def test_forward_launches_the_recorded_kernels(case):
    got = GC.observe(case)
    assert got == GC.EXPECTED[case]
    r = GC.query(case)
    before, section, after = GC.launches(r)
    if GC.CASES[case]["refused"]:
        assert GC.matches(got, (before + section + after)[:len(got)]), r
    elif len(r["chains"]) == 1:
        assert GC.matches(got, before + section + after), r
    else:
        assert GC.matches(got[:len(before)], before) and GC.matches(got[len(got) - len(after):], after), r
