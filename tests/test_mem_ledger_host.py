"""csrc/xsd_ledger.h on the host: the device-memory ledger is plain C++17 without a HIP include, so a stand-alone program
(tests/ledger_host_main.cpp) exercises it with g++ alone: add / remove, a foreign free, the null free, the refusal armed for the n-th
allocation firing exactly once, a disarm, and two threads allocating and freeing concurrently with exact final counters.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc")


def test_ledger_program_passes_every_check(tmp_path):
    exe = tmp_path / "ledger_host"
    cxx = os.environ.get("CXX", "g++")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-pthread", "-I", CSRC, "-o", str(exe),
                    os.path.join(ROOT, "tests", "ledger_host_main.cpp")], check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    lines = p.stdout.splitlines()
    assert p.returncode == 0 and lines[-1] == "PASSED: 0 failure(s)", p.stdout[-3000:]
    assert sum(l.startswith("ok  ") for l in lines) >= 40 and not any(l.startswith("FAIL") for l in lines)


def test_the_ledger_header_needs_no_hip():
    hdr = open(os.path.join(CSRC, "xsd_ledger.h")).read()
    assert not re.search(r"#include\s*<hip|hipMalloc|hipFree|hipError", hdr)


def test_the_allocator_and_the_ledger_are_no_dynamic_symbols():
    """xsd::dev_alloc / dev_free / mem_stats / mem_refuse and class xsd::Ledger are internal to the library (hidden, as xsd::failf is): of
    all this, only the two test entries of include/xsd.h are exported, from the product and from the hooks variant"""
    for lib in ("libxsd_hip.so", "libxsd_hip_hooks.so"):
        path = os.path.join(ROOT, "xmm-superres-denoise_amd", "lib", lib)
        assert os.path.exists(path), f"{path}: build it with `make -C {CSRC}` and `make -C {CSRC} hooks` (__graft_entry__.build() does)"
        names = [l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout.splitlines()]
        assert len(names) > 400
        assert sorted(n for n in names if re.search(r"dev_alloc|dev_free|mem_stats|mem_refuse|Ledger|ledger", n)) == ["xsd_test_mem_refuse", "xsd_test_mem_stats"]
