"""The shared bf16 matrix-core vocabulary of csrc/ (bf16_mma.h, plus lds_barrier in crw_common.h) stays in one place: no .hip
file defines one of its names again, every .hip file that uses one includes the header, and the two instructions that the
header wraps in inline asm / a builtin for a toolchain reason appear as code nowhere else.  Pure text, no GPU, no library."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "radar-sounder-crw_amd", "csrc")
HEADER = "bf16_mma.h"
WRAPPED = ("ds_read_b64_tr_b16", "global_load_lds")


def _code(path):
    """the file's text without comments (string literals are kept: the inline asm lives in them)"""
    with open(path) as f:
        text = f.read()
    pat = r'"(?:\\.|[^"\\])*"|//[^\n]*|/\*.*?\*/'
    return re.sub(pat, lambda m: m.group(0) if m.group(0).startswith('"') else " ", text, flags=re.S)


def _typedefs(code):
    """{name: type text without the name} of the file-scope and local typedefs"""
    out = {}
    for body in re.findall(r"\btypedef\b([^;]*);", code):
        m = re.search(r"(\w+)\s*(?=__attribute__\s*\(\(\s*ext_vector_type)", body) or re.search(r"(\w+)\s*$", body)
        out[m.group(1)] = " ".join((body[:m.start(1)] + body[m.end(1):]).split())
    return out


def _functions(code):
    return set(re.findall(r"__device__\s+inline\s+[\w:]+\s+\**(\w+)\s*\(", code))


def _hip_files():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


HDR = _code(os.path.join(CSRC, HEADER))
COMMON = _code(os.path.join(CSRC, "crw_common.h"))
NAMES = set(_typedefs(HDR)) | _functions(HDR)
SHARED = NAMES | {"lds_barrier"}


def test_the_header_defines_the_vocabulary():
    want = {"bf8", "s4v", "s8v", "u4v", "lds_cp", "f2bf", "bf2f", "bf_lo", "lds_addr_of", "tr_read", "tr_frag", "glds16", "mfma",
            "kc_sw", "kc_off", "rc_sw", "rc_off", "read_frag", "lds_reads_landed"}
    assert want <= NAMES, sorted(want - NAMES)
    assert "lds_barrier" in _functions(COMMON) and "lds_barrier" not in NAMES
    assert re.search(r'#include\s+"crw_common.h"', HDR)


def test_no_kernel_file_defines_a_shared_name_again():
    shared_types = set(_typedefs(HDR).values()) | set(_typedefs(COMMON).values())
    bad = []
    for path in _hip_files():
        code = _code(path)
        for name, body in _typedefs(code).items():
            if name in SHARED or body in shared_types:
                bad.append("%s: typedef %s" % (os.path.basename(path), name))
        for name in SHARED:
            # a definition line: a function specifier in front of the name, and the name's parenthesis the first after it
            if re.search(r"^[^\n;=(]*\b(?:__device__|inline|static|constexpr)\b[^\n;=(]*\b%s\s*\(" % name, code, re.M) or \
                    re.search(r"\busing\s+%s\s*=" % name, code):
                bad.append("%s: %s" % (os.path.basename(path), name))
    assert not bad, bad


def test_every_user_includes_the_header():
    users = 0
    for path in _hip_files():
        code = _code(path)
        used = sorted(n for n in SHARED if re.search(r"(?<![.>\w])%s\b" % n, code))
        if not used:
            continue
        users += 1
        has_hdr = re.search(r'#include\s+"%s"' % re.escape(HEADER), code)
        if set(used) - {"lds_barrier"}:
            assert has_hdr, "%s uses %s without %s" % (os.path.basename(path), used, HEADER)
        else:
            assert has_hdr or re.search(r'#include\s+"crw_common.h"', code), os.path.basename(path)
    assert users >= 7, users  # the files that carried private copies


def test_wrapped_instructions_are_code_in_the_header_only():
    for word in WRAPPED:
        assert word in HDR, word
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if os.path.isfile(path) and os.path.basename(path) != HEADER and not path.endswith("Makefile"):
            code = _code(path)
            for word in WRAPPED:
                assert word not in code, "%s has %s as code: call %s" % (os.path.basename(path), word, HEADER)
