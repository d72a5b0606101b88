"""The two q.k map units share ONE statement of their MFMA fragments, key rows, register-fragment score, write-out and
common entry rules (csrc/ca_qkmap_core.h), checked on the source text: both units include the header, the build watches
it, every shared function and typedef is defined exactly once across the three files, and what the units had of their
own under another prefix is gone."""
import os
import re

from conceptattention_amd.csrc import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conceptattention_amd", "csrc")
UNITS = ("ca_tokmap.hip", "ca_querymap.hip")
HEADER = "ca_qkmap_core.h"
FUNCTIONS = ("qk_mfma", "qk_key_row", "qk_frag_load", "qk_scores", "qk_accumulate", "qk_check", "qk_check_scale_flags")
TYPEDEFS = ("f16x8", "u32x4")
GONE = ("tm_mfma", "qm_mfma", "tm_key_row", "qm_key_row", "tm_q_load", "qm_frag_load", "qm_scores", "shares no code",
        "A kernel family of")
# whether each unit goes through a shared step (ca_tokmap.hip, ca_querymap.hip): tokmap scores rows of its LDS tile with
# qk_mfma itself, querymap register fragments with qk_scores
USES = {"qk_mfma": (True, False), "qk_key_row": (True, True), "qk_frag_load": (True, True), "qk_scores": (False, True),
        "qk_accumulate": (True, True), "qk_check": (True, True), "qk_check_scale_flags": (True, True)}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_both_units_include_the_header_and_the_build_watches_it():
    for unit in UNITS:
        assert '#include "ca_qkmap_core.h"' in _read(unit), unit
        assert unit in build.SOURCES
    assert HEADER in build.HEADERS
    head = _read(HEADER)
    assert "__global__" not in head and "hipLaunchKernelGGL" not in head, "the header adds no kernel and no launch"
    for name in os.listdir(CSRC):           # no other unit includes it: ca_headmap.hip shares none of this arithmetic
        if name.endswith((".hip", ".h", ".inc")) and name not in UNITS:
            assert '#include "ca_qkmap_core.h"' not in _read(name), name


def test_every_shared_name_is_defined_exactly_once_and_used_by_the_units():
    text = {name: _read(name) for name in UNITS + (HEADER,)}
    for fn in FUNCTIONS:        # a definition: a return type, the name, its parameters, an opening brace
        pattern = re.compile(r"^(?:template[^\n]*\n)?[\w \t:<>\*&]*[\w\*&>]\s+\*?" + fn + r"\s*\([^;{}]*\)\s*\{", re.M)
        found = {name: len(pattern.findall(t)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (fn, found)
    for td in TYPEDEFS:
        found = {name: len(re.findall(r"^typedef [^;]*\b" + td + r"\b[^;]*;", t, re.M)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (td, found)
    for fn, used in USES.items():
        got = tuple(bool(re.search(r"\b" + fn + r"\b(?:<[^>]*>)?\(", text[u])) for u in UNITS)
        assert got == used, (fn, got, used)
    for name, t in text.items():
        for word in GONE:
            assert word not in t, (name, word)
    # the write-out and the MFMA builtins are stated in the header alone
    for unit in UNITS:
        assert "__builtin_fmaf(P.weight" not in text[unit] and "__builtin_amdgcn_mfma" not in text[unit], unit
    assert text[HEADER].count("__builtin_fmaf(P.weight, v, P.acc[o])") == 1


def test_what_stays_in_the_units():
    """The kernels, their names, the launch structs and each unit's size rule and differing words; both public structs
    and every macro stay in the units' own headers."""
    tok, qry = _read("ca_tokmap.hip"), _read("ca_querymap.hip")
    assert "void ca_tokmap_kernel(TokmapLaunch A)" in tok and "struct TokmapLaunch {" in tok
    for kernel in ("qm_stats_kernel", "qm_emit_kernel"):
        assert f"void {kernel}(QuerymapLaunch A)" in qry
    assert "struct QuerymapLaunch {" in qry
    assert "tm_scores(" in tok and "tm_tile_load(" in tok, "the LDS key tile and its score step are tokmap's own"
    assert "sizes invalid (nq=%d n0=%d n1=%d n_tok=%d;" in tok and "sizes invalid (nq=%d n0=%d n1=%d;" in qry
    assert '"q, k0 and, with n1 > 0, k1"' in tok and '"q, k1 and, with n0 > 0, k0"' in qry
    assert "sizes invalid" not in _read(HEADER)
    assert "typedef struct ca_tokmap_problem {" in _read("ca_tokmap.h")
    assert "typedef struct ca_querymap_problem {" in _read("ca_querymap.h")
