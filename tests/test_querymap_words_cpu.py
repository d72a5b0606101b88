"""Words without a GPU, on toy tokens: heatmaps.word_groups (sentencepiece pieces and the toy tokenizer's bytes),
heatmaps.word_maps, the look-up rule, and the DAAM class's caption, its twice-named word and its truncated word."""
import pytest
import torch

from conceptattention_amd import heatmaps as HM
from conceptattention_amd.baselines import DAAMFluxSegmentationModel, daam_caption, daam_concept_tokens
from conceptattention_amd.t5 import ToyByteTokenizer

TOK = ToyByteTokenizer()


def test_word_groups_of_sentencepiece_pieces():
    pieces = ["▁a", "▁dra", "gon", "▁on", "▁", "a", "▁rock", ".", "▁"]
    assert HM.word_groups(pieces) == [("a", [0]), ("dragon", [1, 2]), ("on", [3]), ("a", [4, 5]), ("rock.", [6, 7])]
    # pieces in front of the first mark still form a word; a lone mark is no word
    assert HM.word_groups(["un", "do", "▁it"]) == [("undo", [0, 1]), ("it", [2])]
    assert HM.word_groups(["▁"]) == [] and HM.word_groups([]) == []
    # any other token list: every token its own word
    assert HM.word_groups(["cat</w>", "sat</w>"]) == [("cat</w>", [0]), ("sat</w>", [1])]


def test_word_groups_of_the_toy_tokenizers_bytes():
    text = "A dog,  a café Dog."
    tokens = TOK.tokenize(text)
    assert len(tokens) == len(text.encode("utf-8")) and all(len(t) == 1 for t in tokens)
    groups = HM.word_groups(tokens)
    assert [w for w, _ in groups] == ["A", "dog,", "a", "café", "Dog."]            # split at the space byte, UTF-8 rejoined
    assert groups[1][1] == [2, 3, 4, 5] and groups[3][1] == [10, 11, 12, 13, 14]         # (the accent is two bytes)
    covered = sorted(i for _, ix in groups for i in ix)
    assert covered == [i for i, t in enumerate(tokens) if t != " "]                      # every byte but the spaces, once
    assert HM.word_groups(TOK.tokenize("   ")) == []


def test_look_ups_ignore_case_and_surrounding_punctuation():
    groups = HM.word_groups(TOK.tokenize("A dog, a hot dog and a Dog."))
    assert HM.normalize_word("Dog.") == HM.normalize_word("(dog") == "dog"
    assert HM.find_words(groups, "dog") == [[2, 3, 4, 5], [13, 14, 15], [23, 24, 25, 26]]
    assert HM.find_words(groups, "DOG") == HM.find_words(groups, "dog")
    assert HM.find_words(groups, "hot dog") == [[9, 10, 11, 13, 14, 15]]                 # a phrase: consecutive words
    assert HM.find_words(groups, "cat") == [] and HM.find_words(groups, "") == [] and HM.find_words(groups, "do") == []


def test_word_maps_sum_the_tokens_of_a_word():
    tokens = TOK.tokenize("a cat sat")
    groups = HM.word_groups(tokens)
    maps = torch.arange(len(tokens) * 6, dtype=torch.float32).reshape(len(tokens), 2, 3)
    got = HM.word_maps(maps, groups)
    assert tuple(got.shape) == (3, 2, 3)
    assert torch.equal(got[0], maps[0]) and torch.equal(got[1], maps[2] + maps[3] + maps[4])
    assert torch.equal(got[2], maps[6:9].sum(0))
    assert tuple(HM.word_maps(maps, []).shape) == (0, 2, 3)


def test_the_daam_caption_and_a_word_that_appears_twice():
    concepts = ["cat", "hot dog"]
    caption = daam_caption("a cat and a hot dog on grass", concepts)
    assert caption == "a cat and a hot dog on grass,a cat, a hot dog"                    # the reference's format, verbatim
    tokens = TOK.tokenize(caption)
    idx = daam_concept_tokens(tokens, concepts)
    text = lambda ix: "".join(tokens[i] for i in ix)  # noqa: E731
    assert text(idx[0]) == "catcat," and text(idx[1]) == "hotdoghotdog"                  # every occurrence, token order
    assert len(set(idx[0])) == len(idx[0]) == 7


def test_a_truncated_word_raises():
    concepts = ["cat", "grass"]
    caption = daam_caption("x" * 40, concepts)                                           # 40 + ",a cat, a grass" = 55 bytes
    assert len(daam_concept_tokens(TOK.tokenize(caption), concepts)) == 2
    with pytest.raises(ValueError, match="'grass' has no whole occurrence among the caption's 50 tokens"):
        daam_concept_tokens(TOK.tokenize(caption)[:50], concepts)                        # "gras" is left of it
    with pytest.raises(ValueError, match="'cat' has no whole occurrence"):
        daam_concept_tokens(TOK.tokenize(caption)[:44], concepts)
    assert DAAMFluxSegmentationModel.DIRECTIONS == ("image_to_text", "text_to_image")
