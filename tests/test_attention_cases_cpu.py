"""CPU proof that the exact-arithmetic attention cases (tests/attention_cases.py) notice one wrong key.

For every case the GPU file runs, every mutant of the fp64 reference that applies to a sequence
(a dropped or admitted key, a dropped 32-key block, the next sequence's table row, the neighbouring
kv-head) moves that sequence's output by at least 4x the tolerance the GPU test asserts, while an
emulation of the kernels' own arithmetic stays inside it.  No GPU and no kernel runs here.
"""
import pytest
import torch

import attention_cases as AC
from copilot_for_consensus_amd.ops import reference as R
from copilot_for_consensus_amd.runtime.kv_cache import PagedKVCache

MIN_MUTANT_RATIO = 4.0
SINGLE_KEY = ("drop_newest", "drop_oldest", "admit_next", "admit_below")


def _cases():
    out = []
    for p in AC.DECODE_PARAMS:
        key = (p["regime"], p["G"], p["window"], p["fp8"])
        out += [("decode", key + (3,)), ("decode", key + (4,))]
    out += [("prefill", (p["regime"], p["G"], p["window"], p["fp8"])) for p in AC.PREFILL_PARAMS]
    out += [("encoder", (p["regime"], p["D"])) for p in AC.ENCODER_PARAMS]
    return list(dict.fromkeys(out))


def _build(kind, key):
    return {"decode": AC.decode_case, "prefill": AC.prefill_case, "encoder": AC.encoder_case}[kind](*key)


@pytest.mark.parametrize("kind,key", _cases(), ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)))
def test_emulation_inside_and_every_mutant_outside_the_tolerance(kind, key):
    case = _build(kind, key)
    ratio, msg = case.worst(case.emulate())
    print(f"{case.name}: emulation {ratio:.3f} x tolerance")
    assert ratio <= 1.0, msg
    applied = set()
    for s in case.seqs:
        if s.poison:
            continue
        ref = case.seq_reference(s)
        for mutant in AC.MUTANTS:
            mut = case.seq_reference(s, mutant)
            if mut is None:
                continue
            # the encoder lengths that are a multiple of 2 D have an all-zero reference in the codebook
            # regime (each element's +-1 tags cancel): misread heads cannot show there, other lengths do
            if mutant in AC.GATHER_MUTANTS and kind == "encoder" and not ref.any():
                continue
            # levels: a single key more than 6 levels under its row's maximum carries < 2**-6 of the
            # weight by construction; such a key is not required to show
            if case.regime == "levels" and mutant in SINGLE_KEY and case.mutant_weight(s, mutant) < 2.0 ** -6:
                continue
            applied.add(mutant)
            r = float(((mut - ref).abs() / AC.tol(ref)).max())
            print(f"  {s.label} {mutant}: {r:.1f}")
            assert r >= MIN_MUTANT_RATIO, f"{case.name} {s.label}: mutant {mutant} moves the output by only {r:.2f} x tol"
    expect = set(AC.MASK_MUTANTS) | {"head+1"} | ({"next_row"} if kind != "encoder" else set())
    if not case.window and kind != "encoder":
        expect.discard("admit_below")
    if case.window == 1 and kind == "decode":
        expect.discard("drop_block_last_full")      # one visible key: no block is whole
    assert applied == expect, f"{case.name}: mutants never applied: {sorted(expect - applied)}"


def test_inputs_are_exact_in_the_cache_formats_and_poison_is_finite():
    for fp8 in (False, True):
        for regime in ("codebook", "levels"):
            c = AC.decode_case(regime, 4, 33, fp8)
            assert torch.isfinite(c.kc.float()).all() and torch.isfinite(c.vc.float()).all()
            assert 0 <= int(c.bt.min()) and int(c.bt.max()) < c.kc.shape[0] and min(c.ctx) >= 1
            for s in c.seqs[:10]:
                k, v, _ = c.gather(s)
                keys = torch.arange(s.n)
                assert torch.equal(v[:s.n], AC.tagged_v(keys, c.Hkv, c.D, s.table_row))           # survives bf16 / e4m3 and the scales
                assert torch.equal(k[:s.n], AC._key_rows(regime, keys, c.Hkv, c.D, 32, 16 if fp8 else 48, s.n, 4))
                assert (v[s.n:] == AC.POISON_V).all()
                sc = torch.einsum("hd,nhd->hn", c.q[s.row0].double(), k.repeat_interleave(c.G, 1))
                assert torch.equal(sc, (sc / 8).round() * 8)                            # every q.k a multiple of 8
            # every block no table names is poison
            unmapped = sorted(set(range(c.kc.shape[0])) - set(c.bt.flatten().tolist()))
            assert len(unmapped) == 3 and (c.vc[unmapped].float() * c.v_scale == AC.POISON_V).all()


@pytest.mark.parametrize("axes,params", [(AC.DECODE_AXES, AC.DECODE_PARAMS), (AC.PREFILL_AXES, AC.PREFILL_PARAMS),
                                         (AC.ENCODER_AXES, AC.ENCODER_PARAMS)], ids=["decode", "prefill", "encoder"])
def test_case_lists_cover_every_pair_of_axis_values(axes, params):
    names = list(axes)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            seen = {(p[a], p[b]) for p in params}
            assert seen == {(x, y) for x in axes[a] for y in axes[b]}, (a, b)
    assert len(params) <= 60


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float8_e4m3fn], ids=["bf16", "fp8"])
def test_fresh_kv_cache_pool_is_all_zero(dtype):
    """The attention kernels multiply masked weights (exact zeros) into whatever a partially filled
    block or a padding table entry holds, so stale slots must be finite: a fresh pool is zeros."""
    kv = PagedKVCache(2, 5, 2, 128, "cpu", dtype=dtype)
    for t in kv.k + kv.v:
        assert t.dtype == dtype and not t.view(torch.uint8).any()
    assert kv.k[0].shape == (5, 2, R.KV_BLOCK, 128) and kv.v[0].shape == (5, 2, 128, R.KV_BLOCK)
