"""Build and run tests/host_drivers/main.hip: the kernels' schedules replayed on the CPU under AddressSanitizer and UBSan,
one program for every driver body.  The helper modules (jpeg_core_host, jpeg_enc_core_host, resize_core_host,
fm_eval_common, gan_eval_common, quality_common, store_common, rollout_common, plan_common, world_common) pack a body's
cases and parse its report; they or their test modules call `run`.  The program is an ordinary one: it is started as a child process, nothing is preloaded and nothing of it is
loaded into Python."""
import atexit
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "host_drivers", "main.hip")
# the sanitizers go on the host half only: the device half is what ships and never runs here
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
_built = {}                                                  # sanitize -> path of the program


class NoSanitizerRuntime(RuntimeError):
    pass


# the linker's own words for a runtime library that is not there; any other failure is a build break
_RUNTIME_MISSING = re.compile(r"(cannot find|cannot open|unable to find|no such file)[^\n]*libclang_rt\.(asan|ubsan)"
                              r"|libclang_rt\.(asan|ubsan)[^\n]*(cannot find|cannot open|no such file)", re.I)


def _hipcc():
    sys.path.insert(0, os.path.dirname(HERE))
    from ndivplanning_amd import _build
    return _build._hipcc()


def build(sanitize=True):
    """Compile the program, once per process and per `sanitize`, into a directory that is removed at exit; returns its
    path.  Raises NoSanitizerRuntime where the toolchain cannot link the sanitizers' runtimes."""
    if sanitize in _built:
        return _built[sanitize]
    out_dir = tempfile.mkdtemp(prefix="host_driver_")
    atexit.register(shutil.rmtree, out_dir, ignore_errors=True)
    exe = os.path.join(out_dir, "host_driver")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17"] + (SANITIZE if sanitize else [])
    cmd += ["-Wno-unused-value", "-Wno-pass-failed", "-Wno-invalid-offsetof", "-Wno-dangling-else", SOURCE, "-o", exe]
    print("host_driver.build:", " ".join(cmd), flush=True)
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if res.returncode != 0:
        if sanitize and _RUNTIME_MISSING.search(res.stdout):     # the link step did not find the runtimes
            raise NoSanitizerRuntime(res.stdout[-2000:])
        raise RuntimeError("hipcc failed:\n" + res.stdout[-4000:])
    if sanitize:                                             # every test's sanitizing hangs on this one command line
        with open(exe, "rb") as f:
            assert b"__asan_init" in f.read(), "the program was linked without AddressSanitizer's runtime"
    _built[sanitize] = exe
    return exe


def run(name, payload, work_dir, args=(), timeout=900, exe=None, expect=0):
    """Run the driver body `name` on `payload` (bytes: its IN file) in a child process; asserts that it exits with
    status `expect` and no sanitizer report.  Returns the bytes of its OUT file (expect != 0, a refused input: None, OUT
    is not read); both files are removed."""
    src, dst = os.path.join(str(work_dir), name + "_in.bin"), os.path.join(str(work_dir), name + "_out.bin")
    with open(src, "wb") as f:
        f.write(payload)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=86", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe or build(), name, src, dst, *args], env=env, capture_output=True, text=True, timeout=timeout)
    text = p.stdout + p.stderr
    assert "Sanitizer" not in text and "runtime error" not in text, text[-4000:]
    assert p.returncode == expect, (p.returncode, text[-2000:])
    report = None
    if expect == 0:
        with open(dst, "rb") as f:
            report = f.read()
    os.remove(src)
    if os.path.exists(dst):
        os.remove(dst)
    return report
