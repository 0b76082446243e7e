"""CTC forced alignment on the host (chunkformer_amd/align.py:force_align_host) against a brute-force
enumeration of every label sequence, the tie rule on hand-made rows, repeated labels, the edge
shapes, spans / words and the argument errors.  No GPU, no libcfm."""
import itertools

import numpy as np
import pytest
import torch

from chunkformer_amd import align


def _collapse(seq, blank):
    return align.remove_duplicates_and_blank(seq, blank)


def _cases(n=300, seed=20260):
    rng = np.random.default_rng(seed)
    for i in range(n):
        T = int(rng.integers(1, 7))
        L = int(rng.integers(0, 4))
        V = 4
        blank = int(rng.integers(0, V)) if i % 3 == 0 else 0
        toks = [v for v in range(V) if v != blank]
        y = [int(toks[j]) for j in rng.integers(0, len(toks), size=L)]
        x = rng.standard_normal((T, V)) * 2
        lp = torch.log_softmax(torch.from_numpy(x).float(), dim=-1).numpy()
        yield i, lp, y, blank


def _brute(lp, y, blank):
    """Every length-T sequence over the target's tokens plus blank that collapses to y, with its f64
    sum; ordered so that the first best is the tie rule's (never needed on random rows)."""
    T = lp.shape[0]
    alphabet = sorted(set(y) | {blank})
    best, best_seq, n = -np.inf, None, 0
    for seq in itertools.product(alphabet, repeat=T):
        if _collapse(seq, blank) != y:
            continue
        n += 1
        s = 0.0
        for t, v in enumerate(seq):
            s += float(np.float64(lp[t, v]))
        if s > best:
            best, best_seq = s, list(seq)
    return n, best, best_seq


def test_brute_force_enumeration():
    feasible = total = 0
    for i, lp, y, blank in _cases():
        T, L = lp.shape[0], len(y)
        R = sum(1 for a, b in zip(y[1:], y[:-1]) if a == b)
        n, best, seq = _brute(lp, y, blank)
        total += 1
        assert (n > 0) == (T >= L + R), (i, T, y)
        if n == 0:
            with pytest.raises(ValueError):
                align.force_align_host(lp, y, blank)
            assert align.align_host_status(lp, y, blank)[0] == 1
            continue
        feasible += 1
        r = align.force_align_host(lp, y, blank)
        assert r.frames == seq, (i, T, y, blank)
        assert abs(r.score - best) <= 4 * T * 2.0 ** -53 * max(1.0, abs(r.score)), (i, r.score, best)
        assert _collapse(r.frames, blank) == y
        assert r.frame_logp == [float(lp[t, v]) for t, v in enumerate(r.frames)]
        for q, (a, b) in enumerate(r.spans):
            assert all(f == y[q] for f in r.frames[a:b + 1]) and 0 <= a <= b < T
    assert total >= 200 and feasible >= 150


def test_tie_rule_stay_then_step_then_skip():
    lp = np.full((5, 4), -1.5, dtype=np.float32)
    # all equal: every path has the same score; stay before step puts the tokens as late as possible
    # on the way back (the backtrace prefers staying), and the end state is the last blank unless the
    # last token is strictly better
    r = align.force_align_host(lp, [1, 2], 0)
    assert r.frames == [1, 2, 0, 0, 0] and r.score == -7.5
    assert r.spans == [(0, 0), (1, 1)]
    # skip against step on an exact tie: token 1 -> token 2 directly or through the blank
    lp = np.full((3, 4), -1.0, dtype=np.float32)
    r = align.force_align_host(lp, [1, 2], 0)
    assert r.frames == [1, 2, 0]
    # step against skip on an exact tie: token 2 at frame 2 is reached from the blank (-2) or from
    # token 1 (-2); the step wins, so frame 1 is the blank
    lp[1, 2] = -5.0
    r = align.force_align_host(lp, [1, 2], 0)
    assert r.frames == [1, 0, 2] and r.score == -3.0
    lp[1, 2] = -1.0
    # the end state: the last token only when strictly better
    lp = np.full((2, 4), -1.0, dtype=np.float32)
    assert align.force_align_host(lp, [1], 0).frames == [1, 0]
    lp[1, 1] = -0.5
    assert align.force_align_host(lp, [1], 0).frames == [1, 1]
    lp[1, 1] = -1.0
    lp[0, 0] = -0.5      # starting in the blank is strictly better: blank, then the token
    assert align.force_align_host(lp, [1], 0).frames == [0, 1]


def test_repeated_labels_never_skip():
    # the blank between the two 2s is very unlikely, yet the repeat must pass through it
    lp = np.log(np.array([[0.05, 0.05, 0.9], [0.01, 0.04, 0.95], [0.01, 0.04, 0.95], [0.05, 0.05, 0.9]],
                         dtype=np.float32))
    r = align.force_align_host(lp, [2, 2], 0)
    assert _collapse(r.frames, 0) == [2, 2] and 0 in r.frames[1:3]
    # with different labels the same rows skip the blank
    lp2 = lp.copy()
    lp2[2:, 1] = lp[2:, 2]
    lp2[2:, 2] = lp[2:, 1]
    assert align.force_align_host(lp2, [2, 1], 0).frames == [2, 2, 1, 1]
    rng = np.random.default_rng(5)
    for _ in range(50):
        T = int(rng.integers(5, 12))
        lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((T, 3))).float(), -1).numpy()
        r = align.force_align_host(lp, [1, 1, 2], 0)
        a, b = r.spans[0][1], r.spans[1][0]
        assert b - a >= 2 and all(f == 0 for f in r.frames[a + 1:b])


def test_edge_shapes():
    rng = np.random.default_rng(1)
    lp = torch.log_softmax(torch.from_numpy(rng.standard_normal((5, 6))).float(), -1).numpy()
    # T == L + R: the single possible path
    assert align.force_align_host(lp, [1, 1, 2, 3], 0).frames == [1, 0, 1, 2, 3]
    assert align.force_align_host(lp, [1, 2, 3, 4, 5], 0).frames == [1, 2, 3, 4, 5]
    assert align.force_align_host(lp[:3], [4, 4], 0).frames == [4, 0, 4]
    with pytest.raises(ValueError, match="no alignment"):
        align.force_align_host(lp[:2], [4, 4], 0)
    # L = 0: all blanks, the score their sum in frame order
    r = align.force_align_host(lp, [], 2)
    s = 0.0
    for t in range(5):
        s += float(np.float64(lp[t, 2]))
    assert r.frames == [2] * 5 and r.spans == [] and r.score == s
    # T = 1
    assert align.force_align_host(lp[:1], [3], 0).frames == [3]
    assert align.force_align_host(lp[:1], [], 0).frames == [0]
    r = align.force_align_host(lp[:0], [], 0)
    assert r.frames == [] and r.score == 0.0
    with pytest.raises(ValueError):
        align.force_align_host(lp[:0], [1], 0)


def test_spans_token_times_and_words():
    V = 6
    path = [0, 1, 1, 0, 2, 3, 3, 3, 0, 0, 4, 5, 0]
    lp = np.full((len(path), V), -9.0, dtype=np.float32)
    for t, v in enumerate(path):
        lp[t, v] = -0.01
    y = [1, 2, 3, 4, 5]
    r = align.force_align_host(lp, y, 0)
    assert r.frames == path and r.tokens == y
    assert r.spans == [(1, 2), (4, 4), (5, 7), (10, 10), (11, 11)]
    tt = r.token_times()
    assert tt[0] == (1 * 0.08, 3 * 0.08) and tt[2] == (5 * 0.08, 8 * 0.08)
    assert r.token_times(frame_s=1.0)[4] == (11.0, 12.0)
    cd = {0: "<blank>", 1: "▁he", 2: "llo", 3: "▁wor", 4: "l", 5: "d"}
    w = r.words(cd)
    assert [x["word"] for x in w] == ["hello", "wor" + "ld"]
    assert w[0]["start"] == 1 * 0.08 and w[0]["end"] == 5 * 0.08
    assert w[1]["start"] == 5 * 0.08 and w[1]["end"] == 12 * 0.08
    # a first piece without the word mark still opens a word
    assert [x["word"] for x in align.force_align_host(lp, y, 0).words({**cd, 1: "he"})] == ["hello", "world"]


def test_errors_and_reference_signature():
    lp = torch.log_softmax(torch.randn(8, 5, generator=torch.Generator().manual_seed(0)), -1)
    with pytest.raises(ValueError, match="blank"):
        align.force_align_host(lp, [1, 0, 2], 0)
    with pytest.raises(ValueError):
        align.force_align_host(lp, [1, 5], 0)
    with pytest.raises(ValueError):
        align.force_align_host(lp, [-1], 0)
    with pytest.raises(ValueError):
        align.force_align_host(lp, [1], 7)
    with pytest.raises(ValueError, match="finite"):
        bad = lp.clone()
        bad[:, 2] = float("-inf")
        align.force_align_host(bad, [1, 2], 0)
    nan = lp.clone()
    nan[3] = float("nan")
    assert align.align_host_status(nan, [1, 2], 0)[0] == 4
    # the reference's signature on a CPU tensor: the host path
    y = torch.tensor([1, 3, 3])
    frames = align.force_align(lp, y, blank_id=0)
    assert frames == align.force_align_host(lp, [1, 3, 3]).frames and len(frames) == 8
    # a packed batch names the failing utterances after computing the others
    with pytest.raises(ValueError, match=r"\[1\]"):
        align.align_packed(lp, [0, 4], [4, 4], [[1], [2, 2, 2]])
    ok = align.align_packed(lp, [0, 4], [4, 4], [[1], [2, 2]])
    assert ok[1] == align.force_align_host(lp[4:], [2, 2])


def test_long_target_vectorised():
    """S ~ 8,000 states runs in seconds (one numpy pass per frame)."""
    g = torch.Generator().manual_seed(3)
    T, L, V = 4300, 4000, 32
    lp = torch.log_softmax(torch.randn(T, V, generator=g), -1)
    y = torch.randint(1, V, (L,), generator=g).tolist()
    r = align.force_align_host(lp, y, 0)
    assert _collapse(r.frames, 0) == y and len(r.frames) == T
    s = 0.0
    for v in r.frame_logp:
        s += v
    assert abs(s - r.score) <= 4 * T * 2.0 ** -53 * abs(r.score)
