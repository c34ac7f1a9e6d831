"""One way to device memory: every allocation and free of the library goes through xsd::dev_alloc / xsd::dev_free (csrc/xsd_mem.h), so that
the ledger sees all of them.  A hipMalloc( or hipFree( call anywhere under csrc/ outside xsd_mem.hip would be memory the lifetime tests
(tests/test_hip_lifetime.py) cannot account for.  No GPU."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xmm-superres-denoise_amd", "csrc")
RUNTIME_CALL = re.compile(r"\bhip(Malloc|Free)\w*\s*\(")      # hipMalloc, hipFree and their Async / Managed / Host kin


def _code(text: str) -> str:
    """the text without comments and string literals (a message may name the runtime call)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    return re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', text)


def _sources():
    return sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h", ".cpp", ".hpp")))


def test_the_runtime_allocator_is_called_in_one_file_only():
    assert len(_sources()) >= 25
    hits = {f: RUNTIME_CALL.findall(_code(open(os.path.join(CSRC, f)).read())) for f in _sources()}
    assert {f: h for f, h in hits.items() if h} == {"xsd_mem.hip": ["Malloc", "Free"]}


def test_every_family_reaches_the_ledger():
    """the files that allocated before the ledger existed all call it now, and the two new files are built and tracked as dependencies"""
    for f in ("xsd_engine.hip", "xsd_test_entries.hip", "generic_net.hip", "restormer.hip", "swinfir.hip", "swinir.hip", "hat.hip", "fsim.hip",
              "ext_metrics.hip", "loss_kernels.hip", "mfma_stream_probe.hip", "sw_kernels.h", "sw_gemm_s3x.h"):
        src = _code(open(os.path.join(CSRC, f)).read())
        assert "xsd::dev_alloc(" in src and "xsd::dev_free(" in src, f
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bxsd_mem\.hip\b", mk, re.M)
    assert re.search(r"^HDRS :=.*\bxsd_mem\.h\b", mk, re.M) and re.search(r"^HDRS :=.*\bxsd_ledger\.h\b", mk, re.M)


def test_the_ledger_translation_unit_holds_no_device_code():
    src = _code(open(os.path.join(CSRC, "xsd_mem.hip")).read())
    assert "__global__" not in src and "__device__" not in src and "hipLaunchKernelGGL" not in src
