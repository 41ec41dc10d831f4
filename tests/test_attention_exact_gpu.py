"""The attention kernels on exact-arithmetic inputs, against an fp64 softmax, to one bf16 rounding.

The cases (tests/attention_cases.py) make every softmax weight a power of two and tag every key's V
with an output element of its own, so a dropped, leaked or misplaced key, a wrong kv-head or table
row, or a mishandled rescale is a wrong number far outside ``2**-7 |ref| + 2**-16``
(tests/test_attention_cases_cpu.py proves the margin on the CPU).  Cache slots past ``ctx``, blocks
outside the tables, table padding and the encoder's packed neighbours hold finite poison.
"""
import pytest
import torch

import attention_cases as AC
from copilot_for_consensus_amd.ops import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _native_loaded():
    from copilot_for_consensus_amd.ops import _native
    _native.kernels()  # must load: no silent fallback on a GPU box


def _check(case, out, what=""):
    torch.cuda.synchronize()
    ratio, msg = case.worst(out)
    print(f"{case.name}{what}: worst error {ratio:.3f} x tolerance")
    assert ratio <= 1.0, msg + what


def _paged_args(case):
    return [t.to(DEV) for t in (case.q, case.kc, case.vc, case.bt)] + [torch.tensor(case.ctx, dtype=torch.int32,
                                                                                     device=DEV)]


def _scales(case):
    return dict(k_scale=case.k_scale, v_scale=case.v_scale) if case.kc.dtype == AC.F8 else {}


@pytest.mark.parametrize("p", AC.DECODE_PARAMS, ids=AC.case_id)
def test_paged_decode_exact(p):
    """B = 30 (plain loads): ctx 1..1025 in every case, G 1..16, fixed and balanced partitions,
    windows, bf16 and fp8 caches, each pair of values at least once."""
    case = AC.decode_case(p["regime"], p["G"], p["window"], p["fp8"])
    q, kc, vc, bt, cl = _paged_args(case)
    out = K.paged_decode_attention(q, kc, vc, bt, cl, AC.SCALE, part_blocks=p["part_blocks"], window=p["window"],
                                   **_scales(case))
    _check(case, out)


@pytest.mark.parametrize("p", AC.DECODE_PARAMS, ids=AC.case_id)
def test_paged_decode_exact_nontemporal_batch(p):
    """The same cases at B = 40 (the nontemporal instantiation; repeated rows share their physical
    blocks), with shared_blocks absent, 0 and 2."""
    case = AC.decode_case(p["regime"], p["G"], p["window"], p["fp8"], 4)
    assert case.rows >= 32
    q, kc, vc, bt, cl = _paged_args(case)
    for shared in (None, 0, 2):
        sb = None if shared is None else torch.tensor([shared], dtype=torch.int32, device=DEV)
        out = K.paged_decode_attention(q, kc, vc, bt, cl, AC.SCALE, part_blocks=p["part_blocks"], window=p["window"],
                                       shared_blocks=sb, **_scales(case))
        _check(case, out, f" shared_blocks={shared}")


@pytest.mark.parametrize("p", AC.PREFILL_PARAMS, ids=AC.case_id)
def test_prefill_exact(p):
    """Fresh prompts and chunked continuations, rows crossing the 256 / G tile edge, up to 8 key
    tiles; the levels regime drives the deferred rescale below, at and above its threshold."""
    case = AC.prefill_case(p["regime"], p["G"], p["window"], p["fp8"])
    q, kc, vc, bt, cl = _paged_args(case)
    cu = torch.tensor(case.cu, dtype=torch.int32, device=DEV)
    out = K.prefill_attention(q, kc, vc, bt, cu, cl, AC.SCALE, window=p["window"], **_scales(case))
    _check(case, out)


@pytest.mark.parametrize("p", AC.ENCODER_PARAMS, ids=AC.case_id)
def test_encoder_exact(p):
    case = AC.encoder_case(p["regime"], p["D"])
    cu = torch.tensor(case.cu, dtype=torch.int32, device=DEV)
    out = K.encoder_attention(case.qkv.to(DEV), cu, case.Hq, case.D, AC.SCALE, max(AC.ENCODER_LENS))
    _check(case, out)
