"""``sample_rows`` (csrc/kernels/elementwise.hip): one launch with a different sampler per row.

The oracle is the pair of existing kernels: row r must equal ``K.sample`` on that row alone (B = 1,
so batch row 0) with ``seed = seed[r]`` and ``step = [pos[r]]`` -- exactly, no tolerance."""
from __future__ import annotations

import math

import pytest
import torch

from copilot_for_consensus_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
I32 = torch.int32

# greedy; T = 0.7 untruncated; top_k = 1; top_k = 40; top_p = 0.9; min_p = 0.05; all three cuts.
# (the eighth setting, top_k > V, is row 3 of the second set)
SETS = [
    [K.SamplingParams(0.0), K.SamplingParams(0.7), K.SamplingParams(0.8, top_k=1), K.SamplingParams(1.0, top_k=40),
     K.SamplingParams(0.9, top_p=0.9), K.SamplingParams(1.1, min_p=0.05),
     K.SamplingParams(1.3, top_k=5, top_p=0.5, min_p=0.1)],
    [K.SamplingParams(0.0, top_k=3, top_p=0.5), K.SamplingParams(1.5), K.SamplingParams(0.8, top_k=1),
     K.SamplingParams(1.0, top_k=100000), K.SamplingParams(0.9, top_p=0.9), K.SamplingParams(1.1, min_p=0.05),
     K.SamplingParams(1.3, top_k=5, top_p=0.5, min_p=0.1)],
]
SEEDS = [11, 0, 0xFFFFFFFF, 12345, 7, 0x80000001, 99]
POS = [0, 1, 5, 0, 300, 17, 2]
SHAPES = [8, 1000, 32000, 32003]


def _logits(B, V, seed=0):
    g = torch.Generator().manual_seed(1000 * V + seed)
    x = (torch.randn(B, V, generator=g) * 2).to(BF)       # bf16 rounding leaves plenty of exact ties
    return x.cuda()


def _rows(params, seeds, pos, size=None):
    rows = K.SamplerRows(size or len(params), "cuda")
    rows.set_rows(range(len(params)), params, seeds)
    rows.pos[:len(pos)] = torch.tensor(pos, dtype=I32).cuda()
    return rows


def _oracle(logits, params, seeds, pos):
    out = []
    for r, (sp, seed, p) in enumerate(zip(params, seeds, pos)):
        one = torch.full((1,), -1, dtype=I32, device="cuda")
        K.sample(logits[r:r + 1], one, sp, seed, torch.tensor([p], dtype=I32, device="cuda"))
        out.append(int(one[0]))
    return out


_ORACLE: dict = {}


def _case(V, s):
    """Logits [7, V] and the seven oracle ids of parameter set s at POS and at POS + 1 (computed once)."""
    if (V, s) not in _ORACLE:
        x = _logits(7, V)
        _ORACLE[V, s] = (x, _oracle(x, SETS[s], SEEDS, POS), _oracle(x, SETS[s], SEEDS, [p + 1 for p in POS]))
    return _ORACLE[V, s]


@pytest.mark.parametrize("s", [0, 1])
@pytest.mark.parametrize("V", SHAPES)
def test_rows_equal_the_existing_kernels_and_pos_advances(V, s):
    x, want, want_next = _case(V, s)
    rows = _rows(SETS[s], SEEDS, POS)
    out = torch.full((7,), -1, dtype=I32, device="cuda")
    K.sample_rows(x, out, rows, 7)
    assert out.tolist() == want
    assert all(0 <= t < V for t in want)
    assert rows.pos.tolist() == [p + 1 for p in POS]
    K.sample_rows(x, out, rows, 7)                       # the second launch: the oracle at pos + 1
    assert out.tolist() == want_next
    assert rows.pos.tolist() == [p + 2 for p in POS]
    if V >= 1000:                                        # the streams move: not every sampled row repeats
        assert want[1:] != want_next[1:]


@pytest.mark.parametrize("V", SHAPES)
def test_single_row(V):
    x, want0, _ = _case(V, 0)
    _, want1, _ = _case(V, 1)
    for s, want in ((0, want0), (1, want1)):
        for r in range(7):
            rows = _rows([SETS[s][r]], [SEEDS[r]], [POS[r]])
            out = torch.full((1,), -1, dtype=I32, device="cuda")
            K.sample_rows(x[r:r + 1], out, rows, 1)
            assert int(out[0]) == want[r] and rows.pos.tolist() == [POS[r] + 1]


@pytest.mark.parametrize("V", [1000, 32000])
def test_row_independence(V):
    x, want, _ = _case(V, 0)
    perm = [3, 6, 0, 5, 1, 4, 2]
    rows = _rows([SETS[0][i] for i in perm], [SEEDS[i] for i in perm], [POS[i] for i in perm])
    out = torch.full((7,), -1, dtype=I32, device="cuda")
    K.sample_rows(x[perm].contiguous(), out, rows, 7)
    assert out.tolist() == [want[i] for i in perm]
    # row 4 as it was, every other row with another sampler, seed and position
    params = [K.SamplingParams(2.0, top_k=7)] * 7
    params[4] = SETS[0][4]
    rows = _rows(params, [SEEDS[4] if r == 4 else 1 + r for r in range(7)], [POS[4] if r == 4 else 9 for r in range(7)])
    K.sample_rows(x, out, rows, 7)
    assert int(out[4]) == want[4]


def test_defined_edge_cases():
    V = 1000
    x = _logits(8, V, seed=1)
    x[0] = float("nan")
    x[1] = -math.inf
    x[2] = float("nan")
    x[3] = -math.inf
    x[4] = 1.0
    x[4, [17, 400, 993]] = 3.0                     # tied maxima: the lowest index
    x[5] = 0.0                                     # every logit tied
    x[6, 5] = float("nan")
    x[6, 6] = math.inf
    x[7, ::2] = float("nan")
    params = [K.SamplingParams(0.0), K.SamplingParams(0.0), K.SamplingParams(0.9, top_k=40, top_p=0.9, min_p=0.05),
              K.SamplingParams(0.7), K.SamplingParams(0.0), K.SamplingParams(0.0), K.SamplingParams(0.0),
              K.SamplingParams(1.0, top_k=300)]
    rows = _rows(params, list(range(8)), [0] * 8)
    out = torch.full((8,), -1, dtype=I32, device="cuda")
    K.sample_rows(x, out, rows, 8)
    got = out.tolist()
    assert got[:4] == [0, 0, 0, 0]
    assert got[4] == 17 and got[5] == 0 and got[6] == 6
    assert all(0 <= t < V for t in got) and got[7] % 2 == 1
    assert got == _oracle(x, params, list(range(8)), [0] * 8)


def test_untouched_memory():
    V, slots, width = 1000, 12, 5
    x = _logits(width, V, seed=2)
    rows = _rows(SETS[0][:width], SEEDS[:width], POS[:width], size=slots)
    rows.pos[width:] = 777
    before = {f: getattr(rows, f).clone() for f in rows._FIELDS}
    out = torch.full((slots,), -7, dtype=I32, device="cuda")
    K.sample_rows(x, out[:width], rows, width)
    assert out[width:].tolist() == [-7] * (slots - width) and all(0 <= t < V for t in out[:width].tolist())
    assert rows.pos.tolist() == [p + 1 for p in POS[:width]] + [777] * (slots - width)
    for f in rows._FIELDS:
        if f != "pos":
            assert torch.equal(getattr(rows, f), before[f])
    assert out[:width].tolist() == _oracle(x, SETS[0][:width], SEEDS[:width], POS[:width])
    with pytest.raises(ValueError):
        K.sample_rows(x, out[:width], rows, width + 1)
    with pytest.raises(ValueError):
        K.sample_rows(_logits(slots + 1, 8), torch.zeros(slots + 1, dtype=I32, device="cuda"), rows)


@torch.inference_mode()      # as the engines capture: torch's capture touches generator state they made there
def test_graph_capture():
    V = 32000
    x, _, _ = _case(V, 0)
    eager = _rows(SETS[0], SEEDS, POS)
    out = torch.full((7,), -1, dtype=I32, device="cuda")
    want = []
    for _ in range(3):
        K.sample_rows(x, out, eager, 7)
        want.append(out.tolist())
    rows = _rows(SETS[0], SEEDS, POS)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K.sample_rows(x, out, rows, 7)               # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(s)
    rows.pos.copy_(torch.tensor(POS, dtype=I32))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        K.sample_rows(x, out, rows, 7)
    rows.pos.copy_(torch.tensor(POS, dtype=I32))
    got = []
    for _ in range(3):
        g.replay()
        got.append(out.tolist())
    assert got == want and want[0] != want[1]
    assert rows.pos.tolist() == [p + 3 for p in POS]
