"""Every route through DecoderModel.forward_decode, pinned bit for bit and launch for launch.

The other GPU tests compare decode paths with each other; none would notice both sides of a
comparison changing together.  Here each case prefills short prompts, runs ONE forward_decode and
compares with tests/golden/decode_paths.json (recorded on an MI355X, twice, in separate processes):

* the sha256 of the hidden states, of model.logits(hidden) and of all layers' K and V caches;
* the ordered names of the native entry points called during that one step.

Equality, no tolerance.  The weights are the CPU-seeded Q4_K_M-style GGUF of
test_gguf_resident_gpu.py ("small" preset) and a second file whose ffn_up is Q6_K, so gate and up
differ in type; nothing is drawn from a GPU generator."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import pytest
import torch

from copilot_for_consensus_amd.runtime import gguf as G
from test_gguf_resident_gpu import _prefill, _short_lens, _under, _write_q4km

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).parent / "golden" / "decode_paths.json"
Q_ON = {"CFC_DECODE_QGEMV": "1", "CFC_DECODE_QGEMM": "1"}
Q_OFF = {"CFC_DECODE_QGEMV": "0", "CFC_DECODE_QGEMM": "0"}
# K.QGEMV_LDS_BYTES at which B = 4 rows of ffn (4 * 2816 * 2 + 16) no longer fit; 4 rows of hidden (8208) do
SMALL_LDS = 16384

# model -> (GGUF file, resident, construction flags, drop the quantized copies before construction)
MODELS = {
    "bf16-q": ("q4km", "bf16", Q_ON, False),
    "bf16": ("q4km", "bf16", Q_OFF, False),
    "bf16-splitk": ("q4km", "bf16", dict(Q_OFF, CFC_DECODE_GEMM="splitk"), False),
    "bf16-q-splitk": ("q4km", "bf16", {"CFC_DECODE_QGEMM": "1", "CFC_DECODE_GEMM": "splitk"}, False),
    "packed": ("q4km", "bf16", {}, True),
    "quant": ("q4km", "quant", {}, False),
    "mixed-bf16-q": ("mixed", "bf16", Q_ON, False),
    "mixed-quant": ("mixed", "quant", {}, False),
}

# (model, B, decode_path(B), K.QGEMV_LDS_BYTES or None)
CASES = [
    ("bf16-q", 2, "qgemv", None), ("bf16-q", 6, "qgemm", None), ("bf16-q", 33, "qgemm", None),
    ("bf16-q", 130, "dgemm", None),
    ("bf16", 2, "gemv", None), ("bf16", 6, "dgemm", None),
    ("bf16-splitk", 6, "splitk", None), ("bf16-q-splitk", 6, "qgemm", None),
    ("packed", 1, "gemv", None), ("packed", 4, "gemv", None), ("packed", 6, "dgemm", None),
    ("quant", 2, "qgemv", None), ("quant", 6, "qgemm", None), ("quant", 130, "scratch", None),
    ("mixed-bf16-q", 2, "qgemv", None), ("mixed-quant", 2, "qgemv", None),
    ("bf16-q", 4, "qgemv", SMALL_LDS), ("bf16-q", 2, "qgemv", SMALL_LDS),
    ("quant", 4, "qgemv", SMALL_LDS), ("quant", 2, "qgemv", SMALL_LDS),
]


def case_id(case) -> str:
    model, B, path, lds = case
    return f"{model}-B{B}-{path}" + (f"-lds{lds}" if lds else "")


def _write_mixed(path, cfg):
    """_write_q4km's file with ffn_up as Q6_K: the same weights, gate (Q4_K) and up differing in type."""
    write = G.write_llama_gguf

    def with_q6k_up(path, cfg, sd, qtypes, **kw):
        up = {f"blk.{i}.ffn_up.weight": G.Q6_K for i in range(cfg.layers)}
        return write(path, cfg, sd, qtypes=dict(qtypes, **up), **kw)
    G.write_llama_gguf = with_q6k_up
    try:
        _write_q4km(path, cfg)
    finally:
        G.write_llama_gguf = write


class Zoo:
    """The models of MODELS, each built on first use from files written once into ``root``."""

    def __init__(self, root: Path):
        self.root, self.built = root, {}

    def file(self, name: str) -> Path:
        from copilot_for_consensus_amd.models.decoder import get_config
        path = self.root / f"{name}.gguf"
        if not path.exists():
            (_write_mixed if name == "mixed" else _write_q4km)(path, get_config("small"))
        return path

    def model(self, name: str):
        from copilot_for_consensus_amd.models.decoder import DecoderModel, DecoderWeights
        if name not in self.built:
            file, resident, env, drop_quant = MODELS[name]
            w = DecoderWeights.from_gguf(self.file(file), "cuda", resident=resident)
            if drop_quant:
                w.qlayers = w.q_lm_head = None
            self.built[name] = _under(env, lambda: DecoderModel(w))
        return self.built[name]


class _Trace:
    """Pass-through for the native library that records each entry point's name."""

    def __init__(self, lib, names: list):
        self._lib, self._names = lib, names

    def __getattr__(self, name):
        self._names.append(name)
        return getattr(self._lib, name)


def _sha(*tensors) -> str:
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


def observe(zoo: Zoo, case) -> dict:
    """Digests and launch trace of one decode step of ``case`` on a freshly prefilled cache."""
    from copilot_for_consensus_amd.ops import kernels as K
    name, B, path, lds = case
    model = zoo.model(name)
    assert model.decode_path(B) == path
    _, step = _prefill(model, _short_lens(B))
    names, real, real_lds = [], K.kernels, K.QGEMV_LDS_BYTES
    lib = real()
    K.kernels = lambda: _Trace(lib, names)
    if lds:
        K.QGEMV_LDS_BYTES = lds
    # inference mode, as the engine decodes: the library split-K writes into the shared split-K
    # workspace with out=, which an earlier test may have allocated under inference mode
    with torch.inference_mode():
        try:
            hidden = model.forward_decode(**step)
        finally:
            K.kernels, K.QGEMV_LDS_BYTES = real, real_lds
        logits = model.logits(hidden)
    kv = step["kv"]
    return {"hidden": _sha(hidden), "logits": _sha(logits), "k": _sha(*kv.k), "v": _sha(*kv.v), "trace": names}


@pytest.fixture(scope="module")
def zoo(tmp_path_factory):
    return Zoo(tmp_path_factory.mktemp("decode_paths"))


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_fixture_holds_every_hand_written_case(golden):
    """Only a case whose path holds a library GEMM may be absent (it differed between two runs
    of one build when the fixture was recorded)."""
    missing = {case_id(c) for c in CASES} - set(golden)
    assert all("splitk" in m for m in missing), missing


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_decode_step_matches_the_recorded_bits_and_launches(zoo, golden, case):
    want = golden.get(case_id(case))
    if want is None:
        assert "splitk" in case_id(case)
        return
    got = observe(zoo, case)
    assert got["trace"] == want["trace"]
    assert {k: got[k] for k in ("hidden", "logits", "k", "v")} == {k: want[k] for k in ("hidden", "logits", "k", "v")}


def test_mixed_gate_up_falls_back_per_projection(golden):
    """The traces themselves show the fallbacks: gate/up of differing types leave the quantized GEMV
    for the bf16 GEMV, respectively an unpack + the decode GEMM; B = 4 under the small LDS budget does the
    same for down alone."""
    def count(case, entry):
        return golden[case]["trace"].count(entry)
    layers = 4
    assert count("mixed-bf16-q-B2-qgemv", "cfc_gemv") == layers and count("bf16-q-B2-qgemv", "cfc_gemv") == 0
    assert count("mixed-quant-B2-qgemv", "cfc_qunpack") == 2 * layers and count("quant-B2-qgemv", "cfc_qunpack") == 0
    assert count("mixed-quant-B2-qgemv", "cfc_dgemm") == layers
    assert count(f"bf16-q-B4-qgemv-lds{SMALL_LDS}", "cfc_gemv") == layers
    assert count(f"quant-B4-qgemv-lds{SMALL_LDS}", "cfc_qunpack") == layers
    assert count(f"bf16-q-B2-qgemv-lds{SMALL_LDS}", "cfc_gemv") == 0
    assert count(f"quant-B2-qgemv-lds{SMALL_LDS}", "cfc_qunpack") == 0
