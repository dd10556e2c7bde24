"""tests/poison_cases.py under the emulator: every stage's light cases with the allocation cache handing out poisoned blocks
(DADA2HIP_ALLOC_POISON), then once more in the same process on what that run left in the cache, each case held to its stage's own
oracle; the library's fill counters show that the knob was live, and that it is read per call.  Byte 0x5A for every stage, 0xFF as
well for the stages with hash tables or -1-filled lists (poison_cases.EMU_JOBS).  EMU_GUARD=1: every "device" buffer ends at an
inaccessible page, so an index read out of poisoned memory and used as an address stops there with a frame printed.

A (stage, byte) goes to tests/test_gpu_poisoned_memory.py only after it has passed here.

Every job is one subprocess with dada2_amd._lib pointed at the emulated library, as in tests/test_emu_paired.py; the jobs of the
tests that were selected are started side by side on a small pool when the first of them asks, as tests/test_emu.py does for its
own."""
import os
import subprocess
import sys

import pytest

import poison_cases as P
from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def _spawn(lib, stage, byte):
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import poison_cases as P\n"
        "print(P.run_stage(%r, %d))\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), lib, stage, byte)
    env = dict(os.environ, EMU_GUARD="1")
    env.pop(P.KNOB, None)
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)


@pytest.fixture(scope="module")
def jobs(request, emu_lib):   # noqa: F811
    from concurrent.futures import ThreadPoolExecutor
    me = sys.modules[__name__]
    want = [(it.callspec.params["stage"], it.callspec.params["byte"]) for it in request.session.items
            if getattr(it, "module", None) is me and hasattr(it, "callspec")]
    pool = ThreadPoolExecutor(max_workers=max(1, min(6, (os.cpu_count() or 2) // 2)))
    futs = {k: pool.submit(_spawn, emu_lib, *k) for k in want}
    yield futs
    pool.shutdown(wait=False, cancel_futures=True)


def test_the_table_covers_every_stage_and_both_bytes():
    assert len(P.STAGE_NAMES) == 16 and P.BYTES == (0xFF, 0x5A)
    assert {s for s, b in P.EMU_JOBS if b == 0x5A} == set(P.STAGE_NAMES)
    assert {s for s, b in P.EMU_JOBS if b == 0xFF} >= {"derep", "paired", "seqtab", "upload", "worklist"}
    assert {(s, b) for s, b, part in P.GPU_JOBS} >= set(P.EMU_JOBS)
    import primer_cases
    whole = {"primers": primer_cases.CASE_NAMES}
    for s, parts in P.GPU_PARTS.items():   # a stage cut into parts for the device keeps every case, once
        assert sorted(n for part in parts for n in part) == sorted(whole[s]), s
    assert {s for s in P.STAGE_NAMES if P.STAGES[s]["pinned"]} >= {"upload", "filter", "primers", "readqc", "derep"}


@pytest.mark.parametrize("stage,byte", P.EMU_JOBS, ids=["%s-0x%02X" % j for j in P.EMU_JOBS])
def test_emulated_stage_on_poisoned_then_recycled_memory(jobs, emu_lib, stage, byte):   # noqa: F811
    out = jobs.pop((stage, byte)).result() if (stage, byte) in jobs else _spawn(emu_lib, stage, byte)
    assert out.returncode == 0 and out.stdout.rstrip().splitlines()[-1].startswith("ok " + stage), out.stdout[-2000:] + out.stderr[-6000:]
