"""The two text-encoder units share ONE statement of their attention tile, row reductions, elementwise walk, launch sizes
and fp8 row scale (csrc/ca_text_core.h), checked on the source text: both units include the header, the build watches
it, and every shared function and macro is defined exactly once across the three files."""
import os
import re

from conceptattention_amd.csrc import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conceptattention_amd", "csrc")
UNITS = ("ca_t5.hip", "ca_clip.hip")
HEADER = "ca_text_core.h"
FUNCTIONS = ("tx_carve", "tx_attn_lds_bytes", "tx_stage_kv", "tx_load_q", "tx_score_tile", "tx_softmax", "tx_pv",
             "tx_store_o", "tx_block_sum", "tx_block_max", "tx_fp8_row_scale", "tx_row_blocks", "tx_walk8",
             "tx_walk8_blocks")
MACROS = ("TX_D", "TX_LDK")
GONE = ("t5_block_sum", "t5_block_max", "clip_block_sum", "T5_LDK", "CLIP_LDK", "T5_D", "CLIP_D",
        "The layout is ca_t5_attn_kernel's")
# how often each unit goes through a shared step (ca_t5.hip, ca_clip.hip)
USES = {"tx_stage_kv": (1, 1), "tx_load_q": (1, 1), "tx_score_tile": (1, 1), "tx_softmax": (1, 1), "tx_pv": (1, 1),
        "tx_store_o": (1, 1), "tx_carve": (1, 1), "tx_attn_lds_bytes": (1, 1), "tx_block_sum": (2, 2),
        "tx_fp8_row_scale": (2, 0), "tx_row_blocks": (3, 1), "tx_walk8": (2, 2), "tx_walk8_blocks": (2, 2)}


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_both_units_include_the_header_and_the_build_watches_it():
    for unit in UNITS:
        assert '#include "ca_text_core.h"' in _read(unit), unit
        assert unit in build.SOURCES
    assert HEADER in build.HEADERS
    head = _read(HEADER)
    assert "__global__" not in head and "hipLaunchKernelGGL" not in head, "the header adds no kernel and no launch"
    for name in os.listdir(CSRC):           # no other unit includes it
        if name.endswith((".hip", ".h", ".inc")) and name not in UNITS:
            assert '#include "ca_text_core.h"' not in _read(name), name


def test_every_shared_name_is_defined_exactly_once_and_used_by_the_units():
    text = {name: _read(name) for name in UNITS + (HEADER,)}
    for fn in FUNCTIONS:        # a definition: a return type, the name, its parameters, an opening brace
        pattern = re.compile(r"^(?:template[^\n]*\n)?[\w \t:<>\*&]*[\w\*&>]\s+\*?" + fn + r"\s*\([^;{}]*\)\s*\{", re.M)
        found = {name: len(pattern.findall(t)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (fn, found)
    for macro in MACROS:
        found = {name: len(re.findall(r"^#define " + macro + r"\b", t, re.M)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (macro, found)
    for fn, counts in USES.items():
        got = tuple(len(re.findall(r"\b" + fn + r"\b(?:<[^>]*>)?\(", text[u])) for u in UNITS)
        assert got == counts, (fn, got, counts)
    for name, t in text.items():
        for word in GONE:
            assert word not in t, (name, word)
    # the kernels keep their names, the reductions their tree
    assert "void ca_t5_attn_kernel(" in text["ca_t5.hip"] and "void ca_clip_attn_kernel(" in text["ca_clip.hip"]
    assert text[HEADER].count("return (red[0] + red[1]) + (red[2] + red[3]);") == 1
    assert text[HEADER].count("rows of 72 bf16") == 1, "the bank-slot reason is stated once"


def test_the_launch_size_rules_are_stated_once_in_the_header():
    """tests/t5_cases.py, t5_fp8_cases.py and clip_cases.py restate the two caps; the header must still hold them, once,
    and every row-per-workgroup and elementwise launch of the two units goes through them."""
    text = {name: _read(name) for name in UNITS + (HEADER,)}
    assert text[HEADER].count("rows < 65536 ? rows : 65536") == 1
    assert text[HEADER].count("if (blocks > 65536) blocks = 65536;") == 1
    for unit in UNITS:
        assert "65536" not in text[unit], unit
    assert text["ca_t5.hip"].count("dim3(tx_row_blocks(rows))") == 3 and text["ca_clip.hip"].count("dim3(tx_row_blocks(rows))") == 1
    assert len(re.findall(r"dim3\(tx_walk8_blocks\(rows, [CH]\)\)", text["ca_t5.hip"])) == 2
    assert len(re.findall(r"dim3\(tx_walk8_blocks\(rows, [CH]\)\)", text["ca_clip.hip"])) == 2
    assert text["ca_t5.hip"].count("dim3(256)") == 6 and text["ca_clip.hip"].count("dim3(256)") == 4
