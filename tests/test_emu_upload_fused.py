"""The boundary call's fused upload under the emulator (tests/upload_fused_cases.py): the product's own sample_create - one pass
over the rows, chunk copies queued from inside the pass, input errors raised behind it - and the call that does not wait between
create and run, on the CPU, one subprocess per case as in tests/test_emu_host_ends.py, each against the plain-C restatement.
The stride-below case runs with guarded allocations (EMU_GUARD: every device and pinned buffer ends where an inaccessible page
begins), so a write behind a buffer by a row longer than its stated stride ends the process.  The row work itself
(hostsimd.cpp's marshal_rows) is also run as a stand-alone program under the host sanitizers (tools/upload_fused_check.cpp)."""
import os
import shutil
import subprocess
import sys

import pytest

import upload_fused_cases as uc
from test_emu import CXX, ROOT, emu_lib  # noqa: F401  (the module-scoped fixture that builds the emulated library)

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_emu = pytest.mark.skipif(not os.path.exists(CXX), reason="no host clang++ for the emulator build")


def _through_emulator(lib, call, env=None, timeout=900):
    code = (
        "import sys\n"
        "sys.path[:0] = [%r, %r]\n"
        "from dada2_amd import _lib\n"
        "_lib.LIB_PATH = %r\n"
        "import upload_fused_cases as uc\n"
        "print(uc.%s)\n"
    ) % (ROOT, os.path.join(ROOT, "tests"), lib, call)
    e = dict(os.environ)
    e.pop(uc.KNOB, None)
    e.update(env or {})
    out = subprocess.run([sys.executable, "-c", code], env=e, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0 and out.stdout.startswith("ok "), out.stdout[-2000:] + out.stderr[-4000:]
    return out


@needs_emu
@pytest.mark.parametrize("name", sorted(uc.SHAPES))
def test_emulated_upload_shapes_match_the_restatement(emu_lib, name):   # noqa: F811
    _through_emulator(emu_lib, "run_shape(%r)" % name)


@needs_emu
@pytest.mark.parametrize("name", sorted(uc.ERRORS))
def test_emulated_input_errors_keep_their_message_and_order(emu_lib, name):   # noqa: F811
    _through_emulator(emu_lib, "run_error(%r)" % name, env={"EMU_GUARD": "1"} if name == "stride_one_below" else None)


@needs_emu
def test_emulated_boundary_call_equals_the_resident_sample(emu_lib):   # noqa: F811
    _through_emulator(emu_lib, "run_boundary_equals_resident()")


@needs_emu
def test_emulated_two_samples_in_flight_equal_their_single_calls(emu_lib):   # noqa: F811
    _through_emulator(emu_lib, "run_multi_equals_single()")


@needs_emu
def test_emulated_chunks_and_kmer_launches_are_what_the_rows_allow(emu_lib):   # noqa: F811
    """The knob makes the chunks it says (were it ignored, every shape above would still pass), and a chunk with a row outside the
    stated geometry gets no k-mer launch, nor does any chunk behind it."""
    out = _through_emulator(emu_lib, "run_chunk_cases()")
    assert uc.upload_lines(out.stderr) == uc.EXPECTED_UPLOAD_LINES, out.stderr[-4000:]


@needs_emu
@pytest.mark.parametrize("name", sorted(uc.WORKLIST_CASES))
def test_emulated_final_worklist_is_built_on_the_device(emu_lib, name):   # noqa: F811
    _through_emulator(emu_lib, "run_worklist(%r)" % name)


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which(HIPCC)), reason="no hipcc for the host build")
def test_row_work_under_the_host_sanitizers(tmp_path):
    """tools/upload_fused_check.cpp + hostsimd.cpp, plain host C++ built with the address and undefined-behaviour sanitizers: ragged
    rows, every stride from two below to two above the longest read, bad letters and qualities, buffers of exactly the stated size
    with canary rows around them."""
    exe = str(tmp_path / "upload_fused_check")
    subprocess.check_call([HIPCC, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-x", "c++", os.path.join(ROOT, "tools", "upload_fused_check.cpp"),
                           os.path.join(ROOT, "dada2_amd", "csrc", "hostsimd.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "upload_fused_check: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
