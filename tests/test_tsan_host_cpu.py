"""CPU: thread-sanitizer run of the library's host side ("test with TSAN on the host shim").
Every csrc/*.hip is compiled HOST-ONLY with -fsanitize=thread (no device code, no device needed) together with
tests/cpp/tsan_host.cpp, which drives the 16-thread HNSW builder, the parallel per-group k-means, the Workspace pool and
the process-wide tuning switches; the binary must report no data race and equal results."""
import glob
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

from conftest import ROOT

CSRC = os.path.join(ROOT, "lab_1806_vec_db_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# -fno-gpu-sanitize: the sanitizer instruments the host side only, never a device code object
FLAGS = ["-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-fno-gpu-sanitize", "-fPIE", "-DVDB_HOST_SANITIZER_BUILD",
         "-ffp-contract=off", "-fno-fast-math", "-pthread", "-Wno-unused-result"]


def test_host_side_is_race_free_under_tsan(tmp_path):
    srcs = sorted(glob.glob(os.path.join(CSRC, "*.hip"))) + [os.path.join(ROOT, "tests", "cpp", "tsan_host.cpp")]

    def cc(src):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        r = subprocess.run([HIPCC] + FLAGS + ["-c", src, "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, src + "\n" + r.stderr[-3000:]
        return obj

    with ThreadPoolExecutor(6) as pool:
        objs = list(pool.map(cc, srcs))
    # a host-only object still refers to its translation unit's device code object (__hip_fatbin_<hash>, handed to
    # __hipRegisterFatBinary at start-up): give each an empty placeholder -- registration is lazy and nothing here launches
    syms = set()
    for o in objs:
        nm = subprocess.run(["nm", "-u", o], capture_output=True, text=True).stdout
        syms.update(ln.split()[-1] for ln in nm.splitlines() if "__hip_fatbin_" in ln)
    stub = tmp_path / "fatbin_stubs.c"
    stub.write_text("".join(f'__attribute__((section(".hip_fatbin"), aligned(4096))) const char {sy}[4096] = {{0}};\n' for sy in sorted(syms)))
    r = subprocess.run(["gcc", "-c", str(stub), "-o", str(tmp_path / "fatbin_stubs.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    objs.append(str(tmp_path / "fatbin_stubs.o"))
    exe = str(tmp_path / "tsan_host")
    r = subprocess.run([HIPCC, "-fsanitize=thread", "-fno-gpu-sanitize", "-pthread", "-o", exe] + objs + ["-ldl"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 report_signal_unsafe=0 exitcode=66",
               LD_LIBRARY_PATH="/opt/rocm/lib:" + os.environ.get("LD_LIBRARY_PATH", ""))
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=900)
    assert "WARNING: ThreadSanitizer" not in out.stderr, out.stderr[-6000:]
    assert out.returncode == 0 and "tsan_host: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
