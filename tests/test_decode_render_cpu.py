"""CPU: the pieces every decoding mode shares on the Python side -- the row-range check (_lib.packed_ranges), the n-best
unpacking (search.nbest_results) and ChunkFormerModel's render / sentence-split helpers -- on hand-made inputs with the
expected values written out."""
import numpy as np
import pytest
import torch

from chunkformer_amd import _lib, search
from chunkformer_amd import model as M

CHAR_DICT = {3: "▁a", 4: "b", 5: "▁c"}


def _bare_model(char_dict):
    m = M.ChunkFormerModel.__new__(M.ChunkFormerModel)
    m.char_dict = char_dict
    return m


def _result():
    """tokens [3, 4] at frames [1, 5] (of T = 8), with a three-entry n-best"""
    return search.DecodeResult(tokens=[3, 4], score=-0.5, times=[1, 5], nbest=[[3, 4], [3], [5, 4]],
                               nbest_scores=[-0.5, -1.0, -3.0], nbest_times=[[1, 5], [1], [2, 5]])


# ------------------------------------------------------------------------------------ render
def test_render_without_char_dict_returns_the_result():
    r = _result()
    assert _bare_model(None)._render(r, False) is r
    assert _bare_model(None)._render(r, True) is r


def test_render_nbest_and_text():
    m = _bare_model(CHAR_DICT)
    assert m._render(_result(), True) == ["ab", "a", "cb"]
    assert m._render(_result(), False) == "ab"


@pytest.mark.parametrize("silence,segments", [
    # 0.5 s = 6 frames: neither blank run (3 and 2 frames) closes a sentence
    (0.5, [{"decode": "ab", "start": "00:00:00:000", "end": "00:00:00:560"}]),
    # 0.25 s = 3 frames: the run after frame 1 closes "a" at frame 4; "b" starts at frame 5 and runs to the last frame
    (0.25, [{"decode": "a", "start": "00:00:00:000", "end": "00:00:00:320"},
            {"decode": "b", "start": "00:00:00:400", "end": "00:00:00:560"}]),
])
def test_render_segments(silence, segments):
    m = _bare_model(CHAR_DICT)
    assert m._render_segments(_result(), 8, silence, True) == segments
    assert m._render_segments(_result(), 8, silence, False) == " ".join(s["decode"] for s in segments)
    # the composition it stands for: the tokens at their frames in a dense [T, 1] array
    dense = np.zeros((8, 1), dtype=np.int64)
    dense[1, 0], dense[5, 0] = 3, 4
    assert segments == M.format_segments(M.transducer_segments(dense, M.max_silence_frames(silence)), CHAR_DICT)


def test_resolve_decoding_records():
    m = _bare_model(None)
    m.model_type, m.is_classification, m.rescorer, m.rnnt, m.encoder = "asr_model", False, None, None, object()
    assert m._resolve_decoding("ctc_greedy_search") is None
    d = m._resolve_decoding("ctc_prefix_beam_search")
    assert (d.method, d.searcher, d.lens, d.timed) == ("ctc_prefix_beam_search", m.encoder, "ctc", True)
    for method in ("attention_rescoring", "attention", "rnnt_beam_search", "nonsense"):
        with pytest.raises(ValueError):
            m._resolve_decoding(method)


# ------------------------------------------------------------------------------------ n-best unpacking
def _packed():
    """K = 3 planes of 12 rows; utterance 0 at rows [1, 4), utterance 1 at rows [7, 11); 99 / -7 outside the hypotheses"""
    tok = torch.full((3, 12), 99, dtype=torch.int32)
    tim = torch.full((3, 12), -7, dtype=torch.int32)
    tok[0, 1:3], tim[0, 1:3] = torch.tensor([5, 6]), torch.tensor([0, 2])
    tok[0, 7:10], tim[0, 7:10] = torch.tensor([7, 8, 9]), torch.tensor([0, 1, 3])
    tok[2, 7:8], tim[2, 7:8] = torch.tensor([4]), torch.tensor([2])
    lens = torch.tensor([[2, 0, 0], [3, 0, 1]], dtype=torch.int32)
    scores = torch.tensor([[-1.5, 0.0, 0.0], [-0.25, -0.5, -2.0]], dtype=torch.float64)
    counts = torch.tensor([1, 3], dtype=torch.int32)
    return tok, tim, lens, scores, counts, torch.tensor([1, 7], dtype=torch.int32)


def _fields(r):
    return (r.tokens, r.score, r.times, r.nbest, r.nbest_scores, r.nbest_times)


def test_nbest_results():
    tok, tim, lens, scores, counts, starts = _packed()
    a, b = search.nbest_results(tok, tim, lens, scores, counts, starts)
    assert _fields(a) == ([5, 6], -1.5, [0, 2], [[5, 6]], [-1.5], [[0, 2]])
    assert _fields(b) == ([7, 8, 9], -0.25, [0, 1, 3], [[7, 8, 9], [], [4]], [-0.25, -0.5, -2.0], [[0, 1, 3], [], [2]])
    # numpy planes and plain lists are taken too
    c, d = search.nbest_results(tok.numpy(), tim.numpy(), lens.tolist(), scores.tolist(), counts.tolist(), [1, 7])
    assert _fields(c) == _fields(a) and _fields(d) == _fields(b)


def test_nbest_results_without_times():
    tok, _, lens, scores, counts, starts = _packed()
    a, b = search.nbest_results(tok, None, lens, scores, counts, starts)
    assert _fields(a) == ([5, 6], -1.5, None, [[5, 6]], [-1.5], None)
    assert _fields(b) == ([7, 8, 9], -0.25, None, [[7, 8, 9], [], [4]], [-0.25, -0.5, -2.0], None)
    assert search.nbest_results(tok, None, lens[:0], scores[:0], counts[:0], starts[:0]) == []


# ------------------------------------------------------------------------------------ row ranges
def test_packed_ranges():
    rs, rl = _lib.packed_ranges([0, 4], torch.tensor([4, 6]), 10, "encoder rows")
    assert rs.dtype == rl.dtype == torch.int32 and not rs.is_cuda
    assert rs.tolist() == [0, 4] and rl.tolist() == [4, 6]
    rs, rl = _lib.packed_ranges([], [], 0, "encoder rows")
    assert rs.dtype == torch.int32 and rs.numel() == 0 and rl.numel() == 0
    assert [t.tolist() for t in _lib.packed_ranges([3], [0], 3, "top-k arrays")] == [[3], [0]]   # empty range at the end
    for starts, lens in (([-1], [2]),            # a negative start
                         ([0], [-1]),            # a negative length
                         ([0, 4], [4, 7]),       # an overrun
                         ([2 ** 31 - 1], [2]),   # an overrun that int32 arithmetic would wrap
                         ([0, 4], [4])):         # unequal lengths
        with pytest.raises(ValueError, match="row ranges exceed the top-k arrays"):
            _lib.packed_ranges(starts, lens, 10, "top-k arrays")
