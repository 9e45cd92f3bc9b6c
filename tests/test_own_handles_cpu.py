"""Ownership of device resources, without a device: the move-only owners of csrc/hfmi_own.h over a fake choke point (a stand-alone
program under the host compiler's sanitizers), and the rule that nothing else in the library makes or frees a device resource."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hippyflow_amd", "csrc")


def _host_cxx():
    for name in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        exe = name and shutil.which(name)
        if exe:
            return exe
    return None


def test_owners_over_a_fake_choke_point(tmp_path):
    """tests/native/own_handles_test.cpp: moved-from handles are empty, move-assignment / reset / destruction release exactly once, a
    non-owning stream is never released, every outcome of grow, and every acquire is matched by one release at exit."""
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "own_handles_test")
    version = subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    # the sanitizer runtimes inside the program (clang's default), so that it runs as it is, whatever else the process loads
    static_rt = [] if "clang" in version else ["-static-libasan", "-static-libubsan"]
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] + static_rt + [
        "-I" + CSRC, os.path.join(ROOT, "tests", "native", "own_handles_test.cpp"), "-o", exe]
    built = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout
    ran = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert ran.returncode == 0 and "own handles OK" in ran.stdout, ran.stdout


# the eight HIP calls that make or free a device buffer, a pinned buffer, an event or a stream
_RESOURCE_CALL = re.compile(r"\b(hipMalloc|hipFree|hipHostMalloc|hipHostFree|hipEventCreate\w*|hipEventDestroy|hipStreamCreate\w*|hipStreamDestroy)\s*\(")
# type -> (unit, the one function that may delete an object of it)
_DESTROY = {
    "hfmi_ctx": ("hfmi_ctx.hip", "hfmi_ctx_destroy"),
    "hfmi_op": ("hfmi_op.hip", "hfmi_op_destroy"),
    "hfmi_csr": ("hfmi_block.hip", "hfmi_csr_destroy"),
    "hfmi_amg": ("hfmi_amg.hip", "hfmi_amg_destroy"),
    "hfmi_pchol": ("hfmi_pchol.hip", "hfmi_pchol_destroy"),
    "fftcov_state": ("hfmi_fftcov.hip", "fftcov_destroy"),
    "xfer_state": ("hfmi_xfer.hip", "xfer_destroy"),
}


def _strip_comments(text):
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _function_spans(text):
    """(name, first line, last line) of every function defined at namespace scope: a line that starts in column 0 or inside
    `namespace {`, holds `name(` and opens a brace that is closed by a line starting with `}`."""
    spans, lines = [], text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(?!\s|#|\}|namespace|struct|class|enum|typedef|using|template)[^;{]*?\b(~?\w+(?:::~?\w+)?)\s*\(", lines[i])
        j = i
        while m and j < len(lines) and "{" not in lines[j] and ";" not in lines[j]:
            j += 1
        if m and j < len(lines) and "{" in lines[j] and (";" not in lines[j] or lines[j].index("{") < lines[j].index(";")):
            depth, k = 0, j
            while k < len(lines):
                depth += lines[k].count("{") - lines[k].count("}")
                if depth <= 0:
                    break
                k += 1
            spans.append((m.group(1), i, k))
            i = k + 1
        else:
            i += 1
    return spans


def _variables_of(text, type_name):
    """names declared as `type* name`, `type *name` or as the pointee of a unique_ptr<type> anywhere in the unit"""
    names = set(re.findall(r"\b%s\s*\*\s*(?:const\s+)?(\w+)" % type_name, text))
    names |= set(re.findall(r"unique_ptr<\s*%s\b[^>]*>\s*(\w+)" % type_name, text))
    return names


def test_one_home_for_device_resources_and_deletes():
    units = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "hfmi_own.h" in units and "hfmi_own.hip" in units and "hfmi_comm.hip" in units
    stray = []
    for unit in units:
        if unit.startswith("hfmi_own.") or unit == "hfmi_comm.hip":
            continue
        text = _strip_comments(open(os.path.join(CSRC, unit)).read())
        text = re.sub(r'"(?:[^"\\\n]|\\.)*"', '""', text)      # message texts may name a call
        for n, line in enumerate(text.split("\n"), 1):
            if _RESOURCE_CALL.search(line):
                stray.append("%s:%d: %s" % (unit, n, line.strip()))
    assert not stray, "device resources made or freed outside hfmi_own.* / hfmi_comm.hip:\n" + "\n".join(stray)

    # `delete x` of an owned type: only in that type's destroy function (x: any variable, parameter or member declared with the type)
    member_of = {"xfer_state": {"xfer"}, "fftcov_state": {"fc"}}
    wrong = []
    for unit in units:
        text = _strip_comments(open(os.path.join(CSRC, unit)).read())
        spans = _function_spans(text)
        lines = text.split("\n")
        for type_name, (home, destroy) in _DESTROY.items():
            names = _variables_of(text, type_name) | member_of.get(type_name, set())
            for n, line in enumerate(lines):
                for m in re.finditer(r"\bdelete\s+(?:\w+\s*->\s*)*(\w+)\s*;", line):
                    if m.group(1) not in names:
                        continue
                    inside = [name for name, a, b in spans if a <= n <= b]
                    if unit != home or inside != [destroy]:
                        wrong.append("%s:%d: delete of a %s in %s" % (unit, n + 1, type_name, inside or "no function"))
    assert not wrong, "\n".join(wrong)
    # ... and each of those functions is there and does delete
    for type_name, (home, destroy) in _DESTROY.items():
        text = _strip_comments(open(os.path.join(CSRC, home)).read())
        body = [(a, b) for name, a, b in _function_spans(text) if name == destroy]
        assert len(body) == 1, (home, destroy)
        assert re.search(r"\bdelete\b", "\n".join(text.split("\n")[body[0][0]:body[0][1] + 1])), (home, destroy)
