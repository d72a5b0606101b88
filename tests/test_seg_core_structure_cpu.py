"""The scoring units share ONE statement of their arithmetic (csrc/ca_seg_core.h), checked on the source text: every unit
includes the header, the build watches it, and every shared helper, struct and host check is defined exactly once across
the four files."""
import os
import re

from conceptattention_amd.csrc import build

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "conceptattention_amd", "csrc")
UNITS = ("ca_seg.hip", "ca_segtab.hip", "ca_mseg.hip")
HEADER = "ca_seg_core.h"
FUNCTIONS = ("seg_near", "seg_reflect", "seg_ordkey", "seg_scan_excl", "seg_blur_tap", "seg_mask_row", "seg_mask_col",
             "seg_coeff_row", "seg_coeff_col", "seg_load_x", "seg_clean_score", "seg_carve", "seg_mean_lo_hi",
             "seg_add_confusion", "seg_build_entries", "seg_sort_entries", "seg_walk_thresholds", "seg_write_record",
             "seg_check_geometry", "seg_check_blur", "seg_fill_blur", "seg_fill_geom", "seg_npad", "seg_lds_bytes",
             "seg_raise_lds_limit")
STRUCTS = ("SegGeom", "SegRecord", "SegScratch", "SegLds", "SegStats", "SegWalk")
GONE = ("segtab_near", "segtab_reflect", "segtab_ordkey", "segtab_scan_excl", "SegtabRecord", "SEGTAB_THREADS",
        "SEGTAB_WAVES", "SEGTAB_MAX_CELLS", "SEGTAB_SCRATCH_BYTES", "word for word", "step by step")


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_every_unit_includes_the_header_and_the_build_watches_it():
    for unit in UNITS:
        assert '#include "ca_seg_core.h"' in _read(unit), unit
        assert unit in build.SOURCES
    assert HEADER in build.HEADERS
    head = _read(HEADER)
    assert "__global__" not in head and "hipLaunchKernelGGL" not in head, "the header adds no kernel and no launch"


def test_every_shared_name_is_defined_exactly_once():
    text = {name: _read(name) for name in UNITS + (HEADER,)}
    for fn in FUNCTIONS:        # a definition: a return type, the name, its parameters, an opening brace
        pattern = re.compile(r"^(?:template[^\n]*\n)?[\w \t:<>\*&]*[\w\*&>]\s+" + fn + r"\s*\([^;{}]*\)\s*\{", re.M)
        found = {name: len(pattern.findall(t)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (fn, found)
    for st in STRUCTS:
        found = {name: len(re.findall(r"^struct " + st + r"\b[^;]*\{", t, re.M)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (st, found)
    for macro in ("SEG_THREADS", "SEG_WAVES", "SEG_MAX_CELLS", "SEG_SCRATCH_BYTES"):
        found = {name: len(re.findall(r"^#define " + macro + r"\b", t, re.M)) for name, t in text.items()}
        assert found[HEADER] == 1 and sum(found.values()) == 1, (macro, found)
    for name, t in text.items():
        for word in GONE:
            assert word not in t, (name, word)
    # the flag bits one test serves are pinned where they are assumed
    for pair in ("CA_SEGTAB_MEAN_THRESHOLD == CA_SEG_MEAN_THRESHOLD", "CA_SEGTAB_DOWNSCALE == CA_SEG_DOWNSCALE",
                 "CA_SEGTAB_BLUR == CA_SEG_BLUR", "CA_MSEG_BLUR == CA_SEG_BLUR"):
        assert pair in text[HEADER], pair
    assert text[HEADER].count("static_assert(sizeof(SegRecord) == 40") == 1
