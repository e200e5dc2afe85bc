"""The launch rule of DESIGN.md ("Kernel launches"), read off the sources (no GPU): kernels are launched through lm_launch (csrc/launch.h)
alone, every launcher declared in a header returns a [[nodiscard]] hipError_t, and no host unit asks hipGetLastError() what a launch did."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "6dpose_amd", "csrc")


def sources(*patterns):
    paths = sorted(p for pat in patterns for p in glob.glob(os.path.join(CSRC, pat)))
    assert paths, patterns
    return [(os.path.basename(p), open(p, encoding="utf-8").read().splitlines()) for p in paths]


def test_kernels_are_launched_through_the_helper_alone():
    units = sources("*.hip", "*.cpp", "*.h")
    assert len([n for n, _ in units if n.endswith(".hip")]) >= 21 and any(n == "launch.h" for n, _ in units)
    bad = ["%s:%d" % (n, i + 1) for n, lines in units if n != "launch.h" for i, ln in enumerate(lines) if "hipLaunchKernelGGL" in ln or "<<<" in ln]
    assert not bad, bad
    used = [n for n, lines in units if n.endswith(".hip") and any("lm_launch(" in ln for ln in lines)]
    assert len(used) >= 21, used                          # and the units do launch through it


def test_every_launcher_returns_a_checked_status():
    headers = sources("*_kernels.h", "depth_modes.h", "frame_border.h", "icp_device.h")    # the headers between the .hip units and their callers
    assert len(headers) >= 9
    decl = re.compile(r"^\s*(?:\[\[nodiscard\]\]\s+)?(?:static\s+|inline\s+)*([\w:]+)\s+(launch_\w+|upload_normal_lut)\(")
    found, bad = 0, []
    for n, lines in headers:
        for i, ln in enumerate(lines):
            if ln.lstrip().startswith(("void launch_", "bool launch_")):
                bad.append("%s:%d" % (n, i + 1))
            m = decl.match(ln)
            if m and m.group(1) != "return":
                found += 1
                if m.group(1) != "hipError_t" or "[[nodiscard]]" not in ln:
                    bad.append("%s:%d: %s" % (n, i + 1, m.group(2)))
    assert not bad, bad
    assert found >= 50, found                             # the pattern still sees the declarations
    makefile = open(os.path.join(CSRC, "Makefile"), encoding="utf-8").read()
    assert "-Wall" in makefile and "-Wno-unused-result" not in makefile   # the compiler holds [[nodiscard]]


def test_no_host_unit_reads_the_last_error_for_a_launch():
    bad = []
    for n, lines in sources("*.cpp"):
        for i, ln in enumerate(lines):
            if "hipGetLastError" not in ln:
                continue
            code = ln.split("//", 1)[0]
            cleared = re.sub(r"\(void\)\s*hipGetLastError\(\)", "", code)
            if "hipGetLastError" in cleared and "//" not in ln:     # read, and the line does not say which error it can still see
                bad.append("%s:%d" % (n, i + 1))
    assert not bad, bad
