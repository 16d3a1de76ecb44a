"""The fused scan's host plan without a GPU: deequ_amd/csrc/scan_plan.cpp (validation, slot plan, launch geometry,
arena layout) built host-only under ASan + UBSan with tests/sanitize_scan_plan/main.cpp, which checks the plan of
fixed calls field by field and validate_predicate over rejected examples and 20 000 seeded random programs, and
deequ_amd/csrc/call_plans.cpp (the plans of dq_row_outcomes and dq_dict_scan) with it: term order, inline predicates,
source kinds, slots, zero-block layout, staging size, LDS counter copies and every refusal's code and text."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_scan_plan_under_asan_ubsan():
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "a host C++ compiler is needed"
    here = os.path.join(ROOT, "tests", "sanitize_scan_plan")
    csrc = os.path.join(ROOT, "deequ_amd", "csrc")
    out = os.path.join(here, "build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "scan_plan_checks")
    subprocess.run([cxx, "-std=c++17", "-DDQ_HOST_ONLY", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1", "-I", csrc, "-o", exe,
                    os.path.join(here, "main.cpp"), os.path.join(csrc, "scan_plan.cpp"),
                    os.path.join(csrc, "call_plans.cpp")], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0 and "ERROR: AddressSanitizer" not in p.stderr and "runtime error" not in p.stderr, \
        (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "scan_plan_checks: ok" in p.stdout and "FAILED" not in p.stdout
    accepted = int(re.search(r"random programs accepted: (\d+) of 20000", p.stdout).group(1))
    assert accepted >= 200, accepted
