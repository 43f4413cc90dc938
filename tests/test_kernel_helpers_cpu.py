"""The device helpers the kernel sources share are written once, in csrc/estd_device.h: no .hip file defines one of that header's names
again, and the unit-less name ``make_rsrc`` (three bodies with two meanings of its size argument before the header existed) stays gone.
Reads text only: no compiler, no GPU."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "estdepth_amd", "csrc")
HEADER = os.path.join(CSRC, "estd_device.h")


def _code(path):
    """the file without comments (a comment may name a helper)"""
    text = open(path, encoding="utf-8").read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return re.sub(r"//[^\n]*", "", text)


def _function_def(name):
    # a definition or declaration: specifiers and a return type in front of the name, no call syntax ('=', '(', ',', ';') between them
    return re.compile(r"(?:__device__|__host__|inline|static)\b[^;{}()=,]*?[\w>*&]\s+\b%s\s*\(" % re.escape(name))


def _typedef_def(name):
    return re.compile(r"\b(?:typedef\b[^;]*?\b%s\b[^;]*;|using\s+%s\s*=)" % (re.escape(name), re.escape(name)))


def _constant_def(name):
    return re.compile(r"(?:\b(?:constexpr|const)\b[^;=()\n]*?\b%s\s*=|#\s*define\s+%s\b)" % (re.escape(name), re.escape(name)))


def header_names():
    code = _code(HEADER)
    functions = sorted(set(re.findall(r"__device__\s+__forceinline__\s+[^;{}()]*?[\w>*&]\s+(\w+)\s*\(", code)))
    typedefs = sorted(set(re.findall(r"\btypedef\b[^;]*?\b(\w+)\s+__attribute__\s*\(\([^;]*;", code)))
    constants = sorted(set(re.findall(r"\bconstexpr\b[^;=]*?\b(\w+)\s*=", code)))
    return functions, typedefs, constants


def hip_sources():
    found = []
    for base, _, files in os.walk(CSRC):
        found += [os.path.join(base, f) for f in files if f.endswith(".hip")]
    return sorted(found)


def test_the_header_is_parsed():
    functions, typedefs, constants = header_names()
    # the parser misses nothing (a regular expression that matched too little would make the test below pass vacuously): it finds one name per
    # `__forceinline__`, `typedef` and `constexpr` of the header, so a helper added there is guarded without an edit here
    code = _code(HEADER)
    assert len(functions) == len(re.findall(r"\b__forceinline__\b", code)) >= 20, functions
    assert len(typedefs) == len(re.findall(r"\btypedef\b", code)) >= 5, typedefs
    assert len(constants) == len(re.findall(r"\bconstexpr\b", code)) >= 1, constants
    assert {"as_float4", "make_rsrc_f32", "make_rsrc_bytes", "lds_barrier"} <= set(functions) and "u32x4" in typedefs and "OOB_OFFSET" in constants
    assert len(hip_sources()) >= 23 and any(os.sep + "mesh" + os.sep in p for p in hip_sources()) and any(os.sep + "track" + os.sep in p for p in hip_sources())


def test_the_detectors_find_a_copy():
    # the forms the copies had before they moved
    assert _function_def("as_float4").search("__device__ __forceinline__ float4 as_float4(u32x4 v) { float4 f; return f; }")
    assert _function_def("lerpf").search("__device__ inline float lerpf(float a, float b, float f) { return fmaf(f, b - a, a); }")
    assert _function_def("dpp_add_f64").search("template <int CTRL>\n__device__ __forceinline__ double dpp_add_f64(double v)\n{")
    assert _function_def("make_rsrc_f32").search("__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc_f32(const float* base, size_t elems)")
    assert _typedef_def("u32x4").search("typedef unsigned int u32x4 __attribute__((__vector_size__(16)));")
    assert _constant_def("OOB_OFFSET").search("constexpr unsigned OOB_OFFSET = 0xFFFFFF00u;")
    # ... and leave uses alone
    use = "const float4 a = as_float4(__builtin_amdgcn_raw_buffer_load_b128(rs, OOB_OFFSET, 0, 0)); u32x4 h; v = lerpf(lerpf(a, b, f), c, f);"
    assert not _function_def("as_float4").search(use) and not _function_def("lerpf").search(use)
    assert not _typedef_def("u32x4").search(use) and not _constant_def("OOB_OFFSET").search(use)
    assert not _function_def("lerpf").search("__device__ inline float blend(float a)\n{\n    return lerpf(a, a, a);\n}")


@pytest.mark.parametrize("path", hip_sources(), ids=lambda p: os.path.relpath(p, CSRC))
def test_no_source_defines_a_shared_helper(path):
    functions, typedefs, constants = header_names()
    code = _code(path)
    again = [n for n in functions if _function_def(n).search(code)]
    again += [n for n in typedefs if _typedef_def(n).search(code)]
    again += [n for n in constants if _constant_def(n).search(code)]
    assert not again, "%s defines %s: csrc/estd_device.h already does" % (os.path.relpath(path, ROOT), ", ".join(again))


def test_the_grid_search_is_written_once():
    # the private copies of the cell coordinate, the finite test and the grid check the search sources held before they moved
    gone = re.compile(r"\b(?:knn_cell_coord|knn_finite|knn_grid_ok|finite_f|grid_ok)\b")
    for path in hip_sources():
        code = _code(path)
        assert not gone.search(code), "%s: %s" % (os.path.relpath(path, ROOT), gone.search(code).group(0))
        # the ring walk's first line: csrc/estd_device.h has the only one (grid_ring_walk)
        assert "for (int r = 0; r <= r_max" not in code, os.path.relpath(path, ROOT)
    assert _code(HEADER).count("for (int r = 0; r <= r_max") == 1
    # the host side of the checks: one definition each under csrc/
    for name in ("estd_finite", "estd_grid_ok", "estd_search_args"):
        found = []
        for base, _, files in os.walk(CSRC):
            found += [os.path.join(base, f) for f in files if _function_def(name).search(_code(os.path.join(base, f)))]
        assert [os.path.relpath(p, CSRC) for p in found] == ["estd_common.h"], (name, found)
        assert len(_function_def(name).findall(_code(found[0]))) == 1, name


def test_make_rsrc_without_a_unit_is_gone():
    for base, _, files in os.walk(CSRC):
        for f in files:
            text = open(os.path.join(base, f), encoding="utf-8").read()        # comments included
            assert "make_rsrc(" not in text, os.path.join(base, f)
