"""What the four device beam search entries refuse, without a GPU: for every bad argument the status, the complete
message and, with two bad arguments at once, which of them is reported; and the quiet exits.  The calls never reach a
launch, so the pointers are dummies that nobody dereferences (the style of
tests/test_nbest_cpu.py::test_nbest_entry_refuses_bad_arguments_without_a_launch).  The expected strings are those of
the library before the entries shared one launch path: this file pins them through any later change of that path."""
import ctypes

import pytest

ONE = ctypes.c_void_p(16)                                               # never dereferenced: the call is refused first
NAN, INF = float('nan'), float('inf')
HEAD = 'probs sizes B T A blank W log'.split()
LM = 'ngram ngram_cap word word_cap order unit bos eos unk space alpha beta oov'.split()
OUTS = 'labels offsets len score ctc'.split()
ORDER = {                                                               # the arguments by position, include/ds2hip.h
    'batch': HEAD + LM + ['ws', 'ws_bytes'] + OUTS,
    'rows': 'probs sizes utt alpha_r beta_r B R T A blank W log'.split() + [n for n in LM if n not in ('alpha', 'beta')]
            + ['ws', 'ws_bytes'] + OUTS,
    'bias': HEAD + LM + 'trans final states weight ws ws_bytes'.split() + OUTS + ['out_bias'],
    'nbest': HEAD + LM + 'trans final states weight nbest ws ws_bytes'.split() + OUTS + ['out_bias', 'out_count'],
}
WS = 1 * (1 + 4 * 4) * 12                                               # ds2_ctc_beam_ws_bytes(1, 4, 4): 204
GOOD = dict(probs=ONE, sizes=ONE, utt=ONE, alpha_r=ONE, beta_r=ONE, B=1, R=1, T=4, A=5, blank=0, W=4, log=0, ngram=None,
            ngram_cap=0, word=None, word_cap=0, order=1, unit=0, bos=-1, eos=-1, unk=-1, space=-1, alpha=0.0, beta=0.0,
            oov=0.0, trans=ONE, final=ONE, states=3, weight=2.0, nbest=2, ws=ONE, ws_bytes=WS, labels=ONE, offsets=ONE,
            len=ONE, score=ONE, ctc=ONE, out_bias=ONE, out_count=ONE)
CHAR = dict(unit=1, order=3, ngram=ONE, ngram_cap=4)                    # a char LM that passes every check
WORD = dict(CHAR, unit=2, word=ONE, word_cap=4, space=1)                # a word LM that does

RANGE = 'bad argument: B >= 0 && R >= 0 && T >= 0 && blank >= 0 && blank < A && unit >= 0 && unit <= 2'
PTRS = ('bad argument: sizes && out_labels && out_offsets && out_len && out_score && out_ctc_logp && '
        '(probs || T == 0 || B == 0)')
NGRAM = 'bad argument: ngram_table && ngram_cap >= 2 && (ngram_cap & (ngram_cap - 1)) == 0'
WORDS = 'bad argument: unit == 1 || (word_table && word_cap >= 2 && (word_cap & (word_cap - 1)) == 0 && space_id < A)'
SHORT = 'workspace of %d bytes < ds2_ctc_beam_ws_bytes = %d'
STATES = '%d context-graph states are outside 1..32768'
GRAPH_NULL = {'bias': 'bias_trans, bias_final and out_bias must not be NULL',
              'nbest': 'with bias_trans, bias_final and out_bias must not be NULL'}

# (changes, message after "<entry>: "): what every entry refuses, each bad value on its own
SHARED = [
    (dict(W=129), 'beam_width 129 is outside 1..128'),
    (dict(A=0), 'alphabet size 0 is outside 1..128'),
    (dict(A=129), 'alphabet size 129 is outside 1..128'),
    (dict(blank=5), RANGE), (dict(blank=-1), RANGE), (dict(B=-1), RANGE), (dict(T=-1), RANGE), (dict(unit=3), RANGE),
    (dict(CHAR, order=0), 'LM order 0 is outside 1..8'),
    (dict(CHAR, order=9), 'LM order 9 is outside 1..8'),
    (dict(CHAR, ngram=None), NGRAM), (dict(CHAR, ngram_cap=6), NGRAM), (dict(CHAR, ngram_cap=1), NGRAM),
    (dict(WORD, word=None), WORDS), (dict(WORD, word_cap=12), WORDS), (dict(WORD, space=5), WORDS),
    (dict(sizes=None), PTRS), (dict(probs=None), PTRS),
] + [({out: None}, PTRS) for out in OUTS] + [
    (dict(ws_bytes=WS - 1), SHORT % (WS - 1, WS)),
    (dict(ws=None), SHORT % (WS, WS)),
    (dict(WORD, ws_bytes=0), SHORT % (0, WS)),                          # a good LM gets as far as the workspace
    # two at once: the earlier check speaks
    (dict(A=129, blank=200), 'alphabet size 129 is outside 1..128'),
    (dict(unit=3, sizes=None), RANGE),
    (dict(CHAR, labels=None, order=0), PTRS),
    (dict(CHAR, order=9, ngram=None), 'LM order 9 is outside 1..8'),
    (dict(CHAR, ngram_cap=6, ws_bytes=0), NGRAM),
    (dict(WORD, ngram=None, word=None), NGRAM),
    (dict(B=0, W=129), 'beam_width 129 is outside 1..128'),             # no utterances: the checks still run
    (dict(B=0, len=None), PTRS),
]
# beam_width 0: the N-best entry compares its nbest with it before anything else
WIDTH_0 = [(dict(W=0), 'beam_width 0 is outside 1..128'), (dict(W=0, A=0), 'beam_width 0 is outside 1..128'),
           (dict(W=129, A=129), 'beam_width 129 is outside 1..128')]
ROWS = [
    (dict(R=-1), '-1 rows'), (dict(R=-3, utt=None, W=0), '-3 rows'),
    (dict(utt=None), 'utt must not be NULL'), (dict(utt=None, W=0), 'utt must not be NULL'),
    (dict(CHAR, alpha_r=None), 'utt, alpha and beta must not be NULL'),
    (dict(CHAR, beta_r=None), 'utt, alpha and beta must not be NULL'),
    (dict(CHAR, utt=None), 'utt, alpha and beta must not be NULL'),
    (dict(unit=3, alpha_r=None, W=0), 'utt, alpha and beta must not be NULL'),
    (dict(R=2), SHORT % (WS, 2 * WS)), (dict(B=0, ws=None), SHORT % (WS, WS)),   # the workspace is per row
]
GRAPH = [
    (dict(states=0), STATES % 0), (dict(states=-1), STATES % -1), (dict(states=32769), STATES % 32769),
    (dict(weight=NAN), 'the weight nan is not finite'), (dict(weight=INF), 'the weight inf is not finite'),
    (dict(weight=-INF), 'the weight -inf is not finite'),
    (dict(final=None), GRAPH_NULL), (dict(out_bias=None), GRAPH_NULL),
    # two at once: the graph is checked before what all entries share, states before weight before the tables
    (dict(states=0, W=129), STATES % 0), (dict(states=0, weight=NAN, final=None), STATES % 0),
    (dict(weight=NAN, final=None, A=0), 'the weight nan is not finite'), (dict(out_bias=None, A=0), GRAPH_NULL),
]
BIAS_ONLY = [(dict(trans=None), GRAPH_NULL), (dict(trans=None, states=0), STATES % 0)]
NBEST = [(dict(nbest=bad), 'nbest %d is outside 1..beam_width = 4' % bad) for bad in (0, -1, 5, 129)] + [
    (dict(W=0), 'nbest 2 is outside 1..beam_width = 0'),
    (dict(out_count=None), 'out_count must not be NULL'),
    # two at once: nbest, then out_count, then the graph, then what all entries share
    (dict(nbest=0, out_count=None), 'nbest 0 is outside 1..beam_width = 4'),
    (dict(nbest=5, states=0), 'nbest 5 is outside 1..beam_width = 4'),
    (dict(out_count=None, states=0), 'out_count must not be NULL'),
    (dict(nbest=0, A=0), 'nbest 0 is outside 1..beam_width = 4'),
    # without bias_trans the other graph arguments are not looked at: the shared checks speak
    (dict(trans=None, states=0, weight=NAN, final=None, out_bias=None, A=129), 'alphabet size 129 is outside 1..128'),
    (dict(trans=None, states=0, ws_bytes=WS - 1), SHORT % (WS - 1, WS)),
]
CASES = ([(e, c, m) for e in ORDER for c, m in SHARED] + [(e, c, m) for e in ('batch', 'rows', 'bias') for c, m in WIDTH_0]
         + [('rows', c, m) for c, m in ROWS] + [(e, c, m) for e in ('bias', 'nbest') for c, m in GRAPH]
         + [('bias', c, m) for c, m in BIAS_ONLY] + [('nbest', c, m) for c, m in NBEST])


@pytest.fixture(scope='module')
def entries():
    from ds2hip import lib
    so = lib.load()

    def call(entry, changes):
        """(status, message) of the entry called with GOOD's values but for ``changes``."""
        unknown = set(changes) - set(GOOD)
        assert not unknown, unknown
        values = dict(GOOD, **changes)
        rc = getattr(so, 'ds2_ctc_beam_search_' + entry)(*[values[n] for n in ORDER[entry]], None)
        return rc, so.ds2_last_error().decode()
    assert {e: len(lib.SIGNATURES['ds2_ctc_beam_search_' + e][1]) - 1 for e in ORDER} == {e: len(ORDER[e]) for e in ORDER}
    return call


@pytest.mark.parametrize('entry, changes, message', CASES, ids=lambda v: None if isinstance(v, dict) else str(v)[:40])
def test_refusal_status_and_whole_message(entries, entry, changes, message):
    from ds2hip import lib
    if isinstance(message, dict):
        message = message[entry]
    assert entries(entry, changes) == (lib.ERR_ARG, 'ds2_ctc_beam_search_%s: %s' % (entry, message))


def test_quiet_exits(entries):
    # no rows: DS2_OK before any check, whatever else is wrong
    bad = dict(R=0, W=0, A=0, blank=-1, B=-1, T=-1, unit=3, utt=None, sizes=None, ws=None, ws_bytes=0, labels=None)
    assert entries('rows', bad)[0] == 0
    # no utterances: DS2_OK once the shared checks have passed, with no workspace at all
    for entry in ('batch', 'bias', 'nbest'):
        assert entries(entry, dict(B=0, ws=None, ws_bytes=0, probs=None))[0] == 0
    # the N-best entry without bias_trans ignores the other graph arguments and out_bias
    assert entries('nbest', dict(B=0, trans=None, final=None, states=-7, weight=NAN, out_bias=None))[0] == 0
    assert entries('bias', dict(B=0, states=32768))[0] == 0 and entries('nbest', dict(B=0, nbest=4))[0] == 0
