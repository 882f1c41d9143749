"""CPU: the owning device-buffer type of the C-ABI host layer (csrc/cnf_devbuf.h) against a stubbed allocator - tests/host/devbuf_check.cpp
defines hipMalloc / hipFree / hipHostMalloc / hipHostFree itself, so the check needs neither a GPU nor the HIP runtime library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"          # the compiler the library itself is built with (csrc/Makefile), here for host code only


def test_devbuf_owns_each_allocation_exactly_once(tmp_path):
    exe = str(tmp_path / "devbuf_check")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                           "-I", os.path.join(ROOT, "continuousnormalizingflows.jl_amd", "csrc"), "-I", "/opt/rocm/include",
                           os.path.join(ROOT, "tests", "host", "devbuf_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "devbuf ok" in out.stdout, out.stdout + out.stderr
