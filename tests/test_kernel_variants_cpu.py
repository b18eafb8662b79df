"""Every build switch of csrc/smp_kernels.hip still compiles: the device side of the file, front end only (no code
generation: under a second each), with the Makefile's compiler and flags and one switch at a time.  Two switches that
claim the same profiling slots (smp_plan_prof.h) must stop at its #error.  Also held here: the files that
smp_kernels.h's SITE_FILES lists exist (trace and bounds records name a source site by a file's place in it; a site in
an unlisted file does not compile), and no function of smp_kernels.hip, or of a header smp_plan_*.h other than the three
that measure and check, carries an #if on a measuring or checking switch."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "squirrel_motion_planner_amd")
CSRC = os.path.join(PKG, "csrc")

# on / off switches, then the tuning constants at a value other than their default
SWITCHES = ["SMP_TRACE", "SMP_SCAN_PROF", "SMP_CONN_PROF", "SMP_JOB_PROF", "SMP_NEAR_PROF", "SMP_VIA_PROF",
            "SMP_DETAIL_PROF", "SMP_WAIT_PROF", "SMP_RING_CHECK", "SMP_PRE_VERIFY", "SMP_BOUNDS"]
CONSTANTS = ["SMP_NEAR_NBK=8", "SMP_PLAN_CT=16", "SMP_HELPER_SLEEP=4", "SMP_POLL_N=64", "SMP_CONN_WAIT=3000",
             "SMP_TRACE -DSMP_TRACE_IT0=10 -DSMP_TRACE_IT1=50"]


def makefile_vars():
    text = open(os.path.join(PKG, "Makefile")).read()

    def var(name):
        m = re.search(r"^%s\s*\??=\s*(.*)$" % name, text, re.M)
        return m.group(1).strip() if m else ""
    return var("HIPCC"), var("ARCH"), var("FLAGS").replace("$(EXTRA)", "").split()


def syntax_only(defines):
    hipcc, arch, flags = makefile_vars()
    if not os.path.isfile(hipcc):
        pytest.skip("no compiler at %s" % hipcc)
    cmd = [hipcc, "--offload-arch=" + arch] + flags + ["-D" + d for d in defines.split(" -D") if d] + [
        "--offload-device-only", "-fsyntax-only", os.path.join(CSRC, "smp_kernels.hip")]
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300)


@pytest.mark.parametrize("defines", [""] + SWITCHES + CONSTANTS, ids=["default"] + SWITCHES + CONSTANTS)
def test_variant_compiles(defines):
    p = syntax_only(defines)
    assert p.returncode == 0, p.stderr[-3000:]


def test_two_owners_of_the_same_slots_are_refused():
    p = syntax_only("SMP_VIA_PROF -DSMP_WAIT_PROF")
    assert p.returncode != 0
    assert "profiling slots 28..31: at most one of" in p.stderr, p.stderr[-3000:]


MEASURING_HEADERS = ["smp_plan_prof.h", "smp_plan_ringcheck.h", "smp_plan_preverify.h"]


def test_site_table_lists_files_that_exist():
    text = open(os.path.join(CSRC, "smp_kernels.h")).read()
    table = re.findall(r'"([^"]+)"', re.search(r"SITE_FILES\[\] = \{(.*?)\};", text, re.S).group(1))
    assert table[0] == "smp_kernels.hip" and len(table) == len(set(table))
    assert all(os.path.isfile(os.path.join(CSRC, n)) for n in table), table
    assert all(('#include "%s"' % n) in open(os.path.join(CSRC, "smp_kernels.hip")).read() for n in table[1:])


def test_functions_hold_no_measuring_conditionals():
    names = ["smp_kernels.hip"] + sorted(n for n in os.listdir(CSRC)
                                         if n.startswith("smp_plan_") and n.endswith(".h") and n not in MEASURING_HEADERS)
    found = []
    for name in names:
        # brace depth and, per open brace, whether it opened a namespace, a struct / union or anything else (a function
        # body and the blocks in it); a conditional is allowed at file or namespace scope (the smp_debug_* readers, defined
        # per build) and among struct members that exist only in a variant (trole, spc_t, cprof)
        stack = []
        for k, line in enumerate(open(os.path.join(CSRC, name)).read().split("\n"), 1):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line) and any(re.search(r"\b%s\b" % s, line) for s in SWITCHES):
                if "body" in stack:
                    found.append("%s:%d" % (name, k))
            code = re.sub(r"//.*", "", line)
            kind = ("namespace" if re.match(r"\s*namespace\b", code) else
                    "struct" if re.match(r"\s*(struct|union)\b", code) and "body" not in stack else "body")
            for ch in code:
                if ch == "{":
                    stack.append(kind)
                elif ch == "}" and stack:
                    stack.pop()
    assert not found, found
