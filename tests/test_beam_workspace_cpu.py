"""CPU: the workspace totals of the beam searches' byte-count entry points.  The trie regions are carved by one function
(csrc/beam.h) for every search; callers size their buffers from these totals, so they are pinned to the values the
library gave before the regions had one definition (the library loads without a GPU)."""
import pytest

ROWS = (0, 1, 63, 64, 65, 2601)
BEAMS = (1, 10, 16)

# cfm_ctc_beam_workspace_bytes(rows, B, k, with_times, 0): (rows, k) -> (without times, with times)
CTC = {
    (0, 1): (256, 256), (0, 10): (256, 256), (0, 16): (256, 256),
    (1, 1): (1024, 1536), (1, 10): (1024, 1536), (1, 16): (1024, 1536),
    (63, 1): (1280, 1792), (63, 10): (10496, 15616), (63, 16): (16640, 24832),
    (64, 1): (1280, 1792), (64, 10): (10496, 15616), (64, 16): (16640, 24832),
    (65, 1): (2048, 3072), (65, 10): (11264, 16896), (65, 16): (17408, 26112),
    (2601, 1): (42240, 63232), (2601, 10): (416768, 625152), (2601, 16): (666624, 999936),
}

# cfm_op_rnnt_beam_prune_workspace_bytes(T, K): (T, K) -> bytes (the prune operator always keeps times)
PRUNE = {
    (0, 1): 4608, (0, 10): 4608, (0, 16): 4608,
    (1, 1): 4608, (1, 10): 4608, (1, 16): 4608,
    (63, 1): 4864, (63, 10): 18688, (63, 16): 27904,
    (64, 1): 4864, (64, 10): 18688, (64, 16): 27904,
    (65, 1): 6144, (65, 10): 19968, (65, 16): 29184,
    (2601, 1): 66304, (2601, 10): 628224, (2601, 16): 1003008,
}


@pytest.fixture(scope="module")
def lib():
    from chunkformer_amd import _lib
    return _lib


def test_tables_cover_the_grid():
    grid = {(r, k) for r in ROWS for k in BEAMS}
    assert set(CTC) == grid and set(PRUNE) == grid


@pytest.mark.parametrize("k", BEAMS)
@pytest.mark.parametrize("rows", ROWS)
def test_ctc_beam_workspace_bytes(lib, rows, k):
    for B in (1, 70):   # the utterance count does not enter
        assert int(lib.cfm_ctc_beam_workspace_bytes(rows, B, k, 0, 0)) == CTC[rows, k][0]
        assert int(lib.cfm_ctc_beam_workspace_bytes(rows, B, k, 1, 0)) == CTC[rows, k][1]
    assert int(lib.cfm_ctc_beam_workspace_bytes(rows, 1, k, 1, 25)) == CTC[rows, k][1]   # nor do the context nodes


@pytest.mark.parametrize("k", BEAMS)
@pytest.mark.parametrize("T", ROWS)
def test_rnnt_beam_prune_workspace_bytes(lib, T, k):
    assert int(lib.cfm_op_rnnt_beam_prune_workspace_bytes(T, k)) == PRUNE[T, k]


def test_refusals_are_kept(lib):
    for with_times in (0, 1):
        assert int(lib.cfm_ctc_beam_workspace_bytes(4, 1, 0, with_times, 0)) == 0
        assert int(lib.cfm_ctc_beam_workspace_bytes(4, 1, -1, with_times, 0)) == 0
        assert int(lib.cfm_ctc_beam_workspace_bytes(-1, 1, 4, with_times, 0)) == 0
    # the CTC count does not refuse k > 16 (cfm_ctc_beam_search does): it keeps counting
    assert int(lib.cfm_ctc_beam_workspace_bytes(4, 1, 17, 1, 0)) == 3072
    for T, k in ((4, 0), (4, -1), (4, 17), (-1, 4)):
        assert int(lib.cfm_op_rnnt_beam_prune_workspace_bytes(T, k)) == 0
