"""CPU-only: the token automaton of grammar-constrained decoding (grammar.py) -- the constructor's refusals, the sink state, the
host walk, and kern_grammar against an independent plain-Python parser of the rule its docstring states."""
import itertools

import numpy as np
import pytest

from omr_a2s_multimodal_transformer_amd.grammar import Grammar, kern_grammar

EOS = 1


def _three_state():
    """Tokens 0 a, 1 <eos>, 2 b, 3 c (classes 0 a, 1 eos, 2 b|c).  State 0 -a-> 1 -b/c-> 2 -a-> 1; <eos> in states 1 and 2."""
    return Grammar([0, 1, 2, 2], [[1, -1, -1], [-1, 0, 2], [1, 0, -1]], 0, EOS)


# ------------------------------------------------------------------------------------------------ constructor
def test_refuses_a_reachable_state_without_an_allowed_token():
    with pytest.raises(ValueError, match="allows no token"):
        Grammar([0, 1, 0], [[1, -1], [-1, -1]], 0, EOS)
    Grammar([0, 1, 0], [[0, 0], [-1, -1]], 0, EOS)             # the same dead state, unreachable: accepted
    with pytest.raises(ValueError, match="allows no token"):   # a class no vocabulary entry has allows nothing
        Grammar([0, 1, 0], [[1, 0, -1], [-1, -1, 0]], 0, EOS)


def test_refuses_a_reachable_state_that_cannot_reach_an_accepting_one():
    with pytest.raises(ValueError, match="no accepting state"):
        Grammar([0, 1, 2], [[1, 0, 2], [1, -1, -1], [-1, 0, 2]], 0, EOS)      # state 1 loops on itself for ever
    with pytest.raises(ValueError, match="no accepting state"):
        Grammar([0, 1, 0], [[0, -1]], 0, EOS)                                 # <eos> allowed nowhere


def test_refuses_class_ids_and_targets_out_of_range():
    with pytest.raises(ValueError, match="class ids"):
        Grammar([0, 1, 2], [[0, 0]], 0, EOS)
    with pytest.raises(ValueError, match="class ids"):
        Grammar([0, 1, -1], [[0, 0]], 0, EOS)
    with pytest.raises(ValueError, match="targets"):
        Grammar([0, 1, 0], [[1, 0]], 0, EOS)                   # target == S
    with pytest.raises(ValueError, match="targets"):
        Grammar([0, 1, 0], [[-2, 0]], 0, EOS)
    with pytest.raises(ValueError, match="start"):
        Grammar([0, 1, 0], [[0, 0]], 1, EOS)
    with pytest.raises(ValueError, match="classes"):
        Grammar(np.arange(300) % 257, np.zeros((1, 257), dtype=np.int32), 0, EOS)
    with pytest.raises(ValueError, match="class of its own"):
        Grammar([0, 0, 1], [[0, 0]], 0, EOS)
    g = Grammar(np.arange(256), np.zeros((1, 256), dtype=np.int32), 0, EOS)      # 256 classes: the most a table holds
    assert g.C == 256 and g.token_class.dtype == np.uint8 and g.token_class[255] == 255


def test_sink_state():
    g = _three_state()
    assert g.S == 4 and g.sink == 3 and g.next.shape == (4, 3) and g.next.dtype == np.int32
    assert g.next[:, 1].tolist() == [-1, 3, 3, 3]              # every <eos> transition leads to the sink
    assert g.next[3].tolist() == [-1, 3, -1]                   # where only <eos> is allowed
    assert g.walk([0, 1, 1, 1]) == [1, 3, 3, 3]                # a finished row that keeps running keeps a valid state
    assert g.walk([0, 1, 0]) == [1, 3, -1]
    assert g.allowed(3).tolist() == [False, True, False, False]


def test_accepts_prefix_ok_walk():
    g = _three_state()
    assert g.walk([]) == [] and g.prefix_ok([]) and not g.accepts([])
    assert g.walk([0, 2, 0, 3]) == [1, 2, 1, 2]
    assert g.prefix_ok([0, 2, 0, 3]) and not g.accepts([0, 2, 0, 3])
    assert g.accepts([0, 2, 0, 3, 1]) and g.accepts([0, 1])
    assert g.walk([0, 0, 2]) == [1, -1, -1] and not g.prefix_ok([0, 0]) and not g.accepts([0, 0, 1])
    assert not g.accepts([1]) and g.walk([1]) == [-1]          # <eos> is not allowed in the start state
    assert not g.accepts([0, 1, 1])                            # complete means: ends at its first <eos>
    assert g.walk([2], state=1) == [2] and g.walk([7]) == [-1]
    assert g.allowed(1).tolist() == [False, True, True, True]


def test_permissive():
    g = Grammar.permissive(6, EOS, forbid=(0, 2))
    assert g.allowed(g.start).tolist() == [False, True, False, True, True, True]
    assert g.accepts([3, 4, 5, 1]) and not g.prefix_ok([3, 0]) and g.accepts([1])
    assert Grammar.permissive(6, EOS).allowed(0).all()
    with pytest.raises(ValueError):
        Grammar.permissive(6, EOS, forbid=(EOS,))


# ------------------------------------------------------------------------------------------------ kern_grammar
def _parse(words, max_spines, spines):
    """The rule of kern_grammar's docstring, read off a complete word list by splitting it -- no automaton."""
    if not words or words[-1] != "<eos>" or words.count("<eos>") != 1:
        return False
    body = words[:-1]
    if any(w in ("<PAD>", "<pad>", "<sos>") for w in body):
        return False
    seps = ("<con>", "<coc>", "<cor>")
    if not body or len(body) % 2 == 0:
        return False
    if any((w in seps) != (i % 2 == 1) for i, w in enumerate(body)):          # symbol, separator, symbol, ..., symbol
        return False
    if not spines:
        return True
    text = " ".join(body)
    rows = [[voice.split(" <con> ") for voice in row.split(" <coc> ")] for row in text.split(" <cor> ")]
    width = None
    for r, row in enumerate(rows):
        if width is None:
            if not 1 <= len(row) <= max_spines:
                return False
        elif len(row) != width:
            return False
        kinds = ["open" if v == ["*^"] else "close" if v == ["*v"] else "plain" for v in row]
        width = sum(2 if k == "open" else 1 for k in kinds if k != "close")
        width += sum(1 for i, k in enumerate(kinds) if k == "close" and (i == 0 or kinds[i - 1] != "close"))
        if r + 1 < len(rows) and not 1 <= width <= max_spines:
            return False
    return True


@pytest.mark.parametrize("words,max_spines,spines", [
    (["<eos>", "<coc>", "<cor>", "*^", "*v", "n"], 3, True),
    (["<eos>", "<coc>", "<cor>", "<con>", "*v", "n"], 2, True),
    (["<PAD>", "<eos>", "<sos>", "<con>", "<cor>", "n"], 8, False),
])
def test_kern_grammar_equals_a_plain_parser_on_every_sequence_up_to_length_7(words, max_spines, spines):
    w2i = {w: i for i, w in enumerate(words)}
    g = kern_grammar(w2i, max_spines=max_spines, spines=spines)
    accepted = 0
    for n in range(1, 8):
        for ids in itertools.product(range(len(words)), repeat=n):
            if ids[-1] != g.eos:                                # neither side accepts these (asserted for the parser below)
                continue
            want = _parse([words[i] for i in ids], max_spines, spines)
            assert g.accepts(ids) == want, [words[i] for i in ids]
            accepted += want
    assert accepted >= 7                                        # the comparison saw accepted sequences, not only refusals
    assert not _parse(["n", "<coc>", "n"], max_spines, spines) and not g.accepts([w2i["n"]])


W2I = {w: i for i, w in enumerate(["<PAD>", "<eos>", "<sos>", "<con>", "<coc>", "<cor>", "*^", "*v", "4c", "8d", "=", "."])}


def _ids(text):
    return [W2I[w] for w in text.split()]


@pytest.mark.parametrize("text", [
    "4c <coc> 8d <cor> = <coc> = <cor> 8d <coc> . <eos>",                                         # two voices
    "4c <con> 8d <con> 4c <coc> . <cor> 8d <coc> 4c <con> 4c <eos>",                              # a chord with <con>
    "4c <coc> *^ <cor> 4c <coc> 8d <coc> . <cor> = <coc> = <coc> = <eos>",                        # *^ row, then three voices
    "4c <coc> 8d <coc> . <cor> 4c <coc> *v <coc> *v <cor> 8d <coc> 4c <eos>",                     # *v *v row, then two voices
    "4c <eos>",
])
def test_valid_streams_are_accepted(text):
    g = kern_grammar(W2I)
    ids = _ids(text)
    assert g.accepts(ids) and _parse(text.split(), 8, True)
    assert g.walk(ids)[-1] == g.sink and all(g.prefix_ok(ids[:n]) for n in range(len(ids)))


@pytest.mark.parametrize("text,bad_at", [
    ("4c <coc> <cor> 8d <eos>", 2),                           # two separators in a row
    ("<coc> 4c <eos>", 0),                                    # a sequence begins with a symbol
    ("4c <coc> <eos>", 2),                                    # <eos> straight after <coc>
    ("4c <PAD> 8d <eos>", 1),                                 # <pad> in the middle
    ("4c <coc> 8d <cor> <sos> <eos>", 4),                     # <sos> in the middle
    ("4c <coc> 8d <cor> 4c <cor> 8d <eos>", 5),               # a row with too few voices
    ("4c <coc> 8d <cor> 4c <coc> 8d <coc> . <eos>", 7),       # a row with too many voices
    ("4c <coc> 8d <cor> 4c <eos>", 5),                        # <eos> before the last row is complete
    ("4c <coc> *^ <cor> 4c <coc> 8d <cor> . <eos>", 7),       # the row after *^ must hold three voices
    ("*v <coc> *v <cor> 4c <coc> 8d <eos>", 5),               # the row after *v *v holds one voice
])
def test_malformed_streams_are_rejected_at_the_expected_token(text, bad_at):
    g = kern_grammar(W2I)
    states = g.walk(_ids(text))
    assert [s >= 0 for s in states] == [i < bad_at for i in range(len(states))], states
    assert not g.accepts(_ids(text)) and not _parse(text.split(), 8, True)


def test_successor_width_limit_is_enforced_at_cor():
    g = kern_grammar(W2I, max_spines=2)
    ids = _ids("*^ <coc> *^ <cor> 4c <eos>")                   # two *^ voices: the next row would hold four
    assert [s >= 0 for s in g.walk(ids)] == [True, True, True, False, False, False]
    assert g.accepts(_ids("*^ <coc> *^ <eos>"))                # nothing follows the last row
    assert g.accepts(_ids("*^ <coc> *^ <con> 4c <cor> 4c <coc> 4c <coc> 4c <eos>")) is False      # width 3 > 2 as well
    assert g.accepts(_ids("*^ <con> 4c <coc> *^ <con> 4c <cor> 4c <coc> 4c <eos>"))              # both voices made ordinary
    assert [s >= 0 for s in g.walk(_ids("4c <coc> 4c <coc> 4c"))] == [True, True, True, False, False]   # the first row's limit
    with pytest.raises(ValueError):
        kern_grammar({"a": 0})
