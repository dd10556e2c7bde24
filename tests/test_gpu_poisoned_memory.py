"""tests/poison_cases.py on the device: every stage's light cases with the allocation cache handing out blocks filled with 0xFF
and with 0x5A (DADA2HIP_ALLOC_POISON: the whole size class, the slack the streaming kernels read into included), then once more
on what that run left in the cache, each case held to its stage's own oracle.  The library's fill counters
(dada2hip_alloc_poison_stats) show that device blocks - and pinned ones where the stage stages through pinned memory - were
actually filled during the case, and that nothing is filled once the knob is unset again.

Only what has passed under the guarded emulator (tests/test_emu_poisoned_memory.py) is listed in poison_cases.GPU_JOBS."""
import pytest

import poison_cases as P

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("stage,byte,names", P.GPU_JOBS, ids=[P.gpu_job_id(j) for j in P.GPU_JOBS])
def test_stage_on_poisoned_then_recycled_memory_on_the_device(stage, byte, names):
    line = P.run_stage(stage, byte, names)
    print(line)
    assert line.startswith("ok " + stage)
