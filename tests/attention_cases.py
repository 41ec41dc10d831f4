"""Attention test cases whose arithmetic is exact, with an fp64 reference, mutants and a CPU emulation.

Not a test module and no GPU here: ``test_attention_exact_gpu.py`` runs the kernels on these cases,
``test_attention_cases_cpu.py`` proves on the CPU that one wrong key stands far outside the bound.

Why the arithmetic is exact.  The kernels get ``scale = ln(2) / 8``, so ``scale * log2(e)`` is 1/8 up
to fp32 rounding, and q, K are chosen so that every q.k is a multiple of 8: scores in the exp2 domain
are integers and every softmax weight is a power of two -- exact in bf16, as is prefill's pre-scaled
Q.  V holds 0, +-1 and the poison value 8; these and the K entries are exact in bf16 and e4m3, also
after division by the power-of-two cache scales (k_scale 0.5, v_scale 0.25).  P.V and l then
accumulate exactly in fp32; what is left is v_exp's last ulp, the 1/l and the bf16 store, hence

    |out - ref| <= 2**-7 * |ref| + 2**-16

(one bf16 ulp of the stored value, plus the fp32-level terms against |V| <= 1).

Tagged V: ``V[key]`` is +- a one-hot at ``d = key % D`` (sign flips every D keys, with the
kv-head and with the sequence), so every key lands in an output element of its own and a failure names the key.

Two regimes:
  * codebook: ``K[key]`` is row ``(key + 17 * kv_head) % D`` of the D x D Sylvester Hadamard matrix
    and ``q = (64 / D) * H[target + 17 * kv_head]``: keys congruent to the target get weight 256,
    every other key weight 1.  Targets cycle over rows and heads (TARGETS); q = 0 counts keys.
  * levels: ``q = 8 * onehot(d)`` and ``K[key, d]`` a small-integer profile over the keys, constant
    over stretches of one kernel tile (PROFILES), so a head sees flat, rising (below, at and above
    the deferred-rescale threshold of 8), falling, spiking and per-key staircase scores.

Poison (finite, in range): cache slots ``ctx..`` of a last block, pool blocks outside every table,
the block that table padding points to and, for the encoder, short neighbour sequences packed
around each sequence hold keys that score at least a row's maximum, with V = 8 in every element.
"""
from __future__ import annotations

import functools
import itertools
import math
from dataclasses import dataclass, field

import torch

from copilot_for_consensus_amd.ops import reference as R

SCALE = math.log(2) / 8
LOG2E = 1.4426950408889634
TOL_REL, TOL_ABS = 2.0 ** -7, 2.0 ** -16
F8 = torch.float8_e4m3fn
POISON_V = 8.0
KV_BLOCK = R.KV_BLOCK
TARGETS = ("own", "next", "key0", "window_first", "below_window", "mid_block", "zero")
PROFILES = ("flat", "rise3", "rise8", "rise9", "rise20", "fall", "spike_mid", "spike_last", "stair")
NPROF = len(PROFILES)


def tol(ref: torch.Tensor) -> torch.Tensor:
    return TOL_REL * ref.abs() + TOL_ABS


@functools.lru_cache(maxsize=None)
def hadamard(D: int) -> torch.Tensor:
    h = torch.ones(1, 1, dtype=torch.float64)
    while h.shape[0] < D:
        h = torch.cat([torch.cat([h, h], 1), torch.cat([h, -h], 1)], 0)
    assert h.shape[0] == D
    return h


def pairwise(axes: dict[str, list]) -> list[dict]:
    """Deterministic greedy covering array: every value of every axis meets every value of every
    other axis in at least one returned combination."""
    names = list(axes)
    todo = {(a, va, b, vb) for a, b in itertools.combinations(names, 2) for va in axes[a] for vb in axes[b]}
    product = [dict(zip(names, vals)) for vals in itertools.product(*axes.values())]
    out, used = [], {(a, v): 0 for a in names for v in axes[a]}
    while todo:
        def gain(c):      # most new pairs; among equals the values used least so far, then product order
            return (sum((a, c[a], b, c[b]) in todo for a, b in itertools.combinations(names, 2)),
                    -sum(used[a, c[a]] for a in names))
        best = max(product, key=gain)
        todo -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(names, 2)}
        for a in names:
            used[a, best[a]] += 1
        out.append(best)
    return out


def level_profiles(keys: torch.Tensor, stretch: int, L: int, n: int) -> torch.Tensor:
    """[len(keys), NPROF] integer score levels 0..L of PROFILES for a sequence of n keys."""
    s = keys // stretch
    last = (n - 1) // stretch

    def rise(step):
        return (min(step, L) * s) % (L + 1)

    cols = [torch.full_like(keys, L // 2), rise(3), rise(8), rise(9), rise(20), (L - 3 * s).clamp(min=0),
            torch.where(s == (last + 1) // 2, L, 0), torch.where(s == last, L, 0), (keys // 4) % 17]
    return torch.stack(cols, -1).double()


def tagged_v(keys: torch.Tensor, heads: int, D: int, seq: int = 0) -> torch.Tensor:
    """[len(keys), heads, D]: +-onehot(key % D), sign (-1)^(key // D + head + seq): the sign also
    tells the kv-head and, between neighbouring rows of a block table, the sequence."""
    v = torch.zeros(len(keys), heads, D, dtype=torch.float64)
    for h in range(heads):
        v[torch.arange(len(keys)), h, keys % D] = 1.0 - 2.0 * (((keys // D) + h + seq) % 2).double()
    return v


def _key_rows(regime, keys, heads, D, stretch, L, n, head_step):
    """K [len(keys), heads, D] of real keys."""
    k = torch.zeros(len(keys), heads, D, dtype=torch.float64)
    for h in range(heads):
        if regime == "codebook":
            k[:, h] = hadamard(D)[(keys + 17 * h) % D]
        else:
            prof = level_profiles(keys, stretch, L, n)
            k[:, h, :NPROF] = prof[:, [(d + head_step * h) % NPROF for d in range(NPROF)]]
    return k


def _poison_rows(regime, keys, heads, D, L):
    """K of poison slots: the codebook row of the slot's position (a row aiming there scores 64,
    any other row 0, the score of its own ordinary keys), or the top level in every dimension."""
    if regime == "codebook":
        return torch.stack([hadamard(D)[(keys + 17 * h) % D] for h in range(heads)], 1)
    return torch.full((len(keys), heads, D), float(L), dtype=torch.float64)


def _target_key(name, pos, window):
    lo = max(0, pos - window + 1) if window else 0
    mid = (pos // 64) * 32 + 13
    mid = mid if mid <= pos else pos // 2
    return {"own": pos, "next": pos + 1, "key0": 0, "window_first": lo,
            "below_window": lo - 1 if lo > 0 else mid, "mid_block": mid, "zero": None}[name]


def _query(regime, idx, head, G, kvh, pos, window, D, flat=False, head_step=4):
    """q row of query head ``head`` (kv-head kvh) at position pos; idx walks TARGETS / PROFILES.
    flat: in the levels regime take the flat profile (every row gets one such head, so every key of
    the row carries full weight somewhere)."""
    q = torch.zeros(D, dtype=torch.float64)
    if regime == "levels":
        q[(-head_step * kvh) % NPROF if flat else idx % NPROF] = 8.0      # K dim d of kv-head kvh: profile d + head_step * kvh
        return q
    name = TARGETS[idx % len(TARGETS)]
    if G >= 2 and head % G == G - 1:
        name = "zero"                # one pure key count per kv-group
    t = _target_key(name, pos, window)
    if t is not None:
        q = (64.0 / D) * hadamard(D)[(t + 17 * kvh) % D]
    return q.clone()


@dataclass
class Seq:
    row0: int                  # output rows [row0, row0 + m)
    m: int
    n: int                     # ctx (paged) or sequence length (encoder)
    pos: torch.Tensor          # [m] newest visible key of each row
    table_row: int = 0         # paged: row of the block table
    beg: int = 0               # encoder: first packed token
    label: str = ""
    poison: bool = False       # encoder: a poison neighbour (V = 8 everywhere: its own output is 8)


@dataclass
class Case:
    kind: str                  # decode | prefill | encoder
    name: str
    regime: str
    D: int
    Hq: int
    Hkv: int
    window: int = 0
    k_scale: float = 1.0
    v_scale: float = 1.0
    q: torch.Tensor = None     # bf16 [rows, Hq, D]; encoder: view into qkv
    kc: torch.Tensor = None
    vc: torch.Tensor = None
    bt: torch.Tensor = None
    ctx: list = None
    cu: list = None
    qkv: torch.Tensor = None
    seqs: list = field(default_factory=list)
    _memo: dict = field(default_factory=dict, repr=False)

    @property
    def G(self):
        return self.Hq // self.Hkv

    @property
    def rows(self):
        return self.q.shape[0]

    # ---- keys a sequence could read: its own, and what lies just past them
    def gather(self, s: Seq, variant: str = "base"):
        """(K, V [n_all, Hkv, D] fp64 as the kernel would dequantize them, off): key j of the
        result is logical key j - off.  variant: base | next_row | head+1."""
        key = (id(s), variant)
        if key in self._memo:
            return self._memo[key]
        if self.kind == "encoder":
            T = self.qkv.shape[0]
            x = self.qkv.view(T, 3, self.Hq, self.D)
            a, b = max(0, s.beg - 2), min(T, s.beg + s.n + 2)
            k, v, off = x[a:b, 1].double(), x[a:b, 2].double(), s.beg - a
        else:
            row = s.table_row if variant != "next_row" else (s.table_row + 1) % self.bt.shape[0]
            nb = min(self.bt.shape[1], (s.n + KV_BLOCK - 1) // KV_BLOCK + 1)
            k, v = R.gather_kv(self.kc, self.vc, self.bt[row], nb * KV_BLOCK, self.k_scale, self.v_scale)
            k, v, off = k.double(), v.double(), 0
        if variant == "head+1":
            k, v = k.roll(1, 1), v.roll(1, 1)
        self._memo[key] = (k, v, off)
        return self._memo[key]

    def mask(self, s: Seq, mutant: str = "none"):
        """[m, n_all] visibility under ``mutant`` (MASK_MUTANTS), or None where it changes nothing."""
        k, _, off = self.gather(s)
        keys = torch.arange(k.shape[0]) - off
        pos = s.pos[:, None]
        lo = (pos - self.window + 1).clamp(min=0) if self.window else torch.zeros_like(pos)
        base = (keys >= lo) & (keys <= pos)
        if mutant == "none":
            return base
        if mutant == "drop_newest":
            mk = base & ~(keys == pos)
        elif mutant == "drop_oldest":
            mk = base & ~(keys == lo)
        elif mutant == "admit_next":
            mk = base | (keys == pos + 1)
        elif mutant == "admit_below":
            mk = base | (keys == lo - 1)
        else:
            vis = keys[base.any(0)]
            blocks = list(range(int(vis.min()) // KV_BLOCK, int(vis.max()) // KV_BLOCK + 1))
            full = [b for b in blocks if base[:, (keys // KV_BLOCK == b) & (keys >= 0)].any(0).all()
                    and ((keys // KV_BLOCK == b) & (keys >= 0)).sum() == KV_BLOCK]
            b = {"drop_block_first": blocks[0], "drop_block_mid": blocks[len(blocks) // 2],
                 "drop_block_last_full": full[-1] if full else None}[mutant]
            if b is None:
                return None
            mk = base & ~(keys // KV_BLOCK == b)
        return None if torch.equal(mk, base) else mk

    def _scores(self, s: Seq, variant):
        key = (id(s), variant, "s")
        if key not in self._memo:
            k, _, _ = self.gather(s, variant)
            q = self.q[s.row0:s.row0 + s.m].double()
            self._memo[key] = torch.einsum("mhd,nhd->hmn", q, k.repeat_interleave(self.G, 1)) * SCALE
        return self._memo[key]

    def mutant_weight(self, s: Seq, mutant: str) -> float:
        """Largest softmax weight, relative to its row's maximum, of a key that a mask mutant drops
        or admits (over rows and heads): 1.0 for a key at the row's top score."""
        base, mk = self.mask(s), self.mask(s, mutant)
        sc = self._scores(s, "base") / math.log(2)
        top = sc.masked_fill(~(base | mk)[None], float("-inf")).max(-1, keepdim=True).values
        return float(torch.exp2(sc - top).masked_fill(~(base ^ mk)[None], 0.0).max())

    def seq_reference(self, s: Seq, mutant: str = "none"):
        """fp64 softmax attention [m, Hq, D] of one sequence, or None where the mutant does not apply."""
        variant = mutant if mutant in GATHER_MUTANTS else "base"
        if variant != "base":
            if self.kind == "encoder" and variant == "next_row":
                return None
            k0, v0, _ = self.gather(s)
            k1, v1, _ = self.gather(s, variant)
            if torch.equal(k0, k1) and torch.equal(v0, v1):
                return None
        mk = self.mask(s, "none" if variant != "base" else mutant)
        if mk is None:
            return None
        sc = self._scores(s, variant).masked_fill(~mk[None], float("-inf"))
        v = self.gather(s, variant)[1].repeat_interleave(self.G, 1)
        p = torch.nan_to_num(torch.softmax(sc, -1), nan=0.0)      # a mutant may leave a row no key: output 0
        return torch.einsum("hmn,nhd->mhd", p, v)

    def reference(self) -> torch.Tensor:
        if "ref" not in self._memo:
            self._memo["ref"] = torch.cat([self.seq_reference(s) for s in self.seqs], 0)
        return self._memo["ref"]

    # ---- the kernels' arithmetic on the CPU: fp32 scale product (decode) or bf16 pre-scaled Q
    # (prefill, encoder), fp32 exp2, weights rounded to bf16 for P.V, fp32 accumulation, l from the
    # unrounded weights, round-to-nearest bf16 store
    def emulate(self) -> torch.Tensor:
        f32 = torch.float32
        sl2 = (torch.tensor(SCALE, dtype=f32) * torch.tensor(self.k_scale, dtype=f32)) * torch.tensor(LOG2E, dtype=f32)
        outs = []
        for s in self.seqs:
            k, v, _ = self.gather(s)
            k = (k / self.k_scale).to(f32).repeat_interleave(self.G, 1)
            v = (v / self.v_scale).to(f32).repeat_interleave(self.G, 1)
            q = self.q[s.row0:s.row0 + s.m].to(f32)
            if self.kind == "decode":
                sc = torch.einsum("mhd,nhd->hmn", q, k) * sl2
            else:
                sc = torch.einsum("mhd,nhd->hmn", (q * sl2).bfloat16().to(f32), k)
            sc = sc.masked_fill(~self.mask(s)[None], float("-inf"))
            w = torch.exp2(sc - sc.max(-1, keepdim=True).values)
            o = torch.einsum("hmn,nhd->mhd", w.bfloat16().to(f32), v)
            l = w.sum(-1).permute(1, 0)[..., None]
            outs.append((o * torch.tensor(self.v_scale, dtype=f32) / l).bfloat16())
        return torch.cat(outs, 0)

    # ---- comparison
    def seq_of_row(self, row: int) -> Seq:
        return next(s for s in self.seqs if s.row0 <= row < s.row0 + s.m)

    def worst(self, out: torch.Tensor):
        """(largest error / tolerance, message naming case, row, head, element and tagged key)."""
        ref = self.reference()
        out = out.detach().double().cpu().view_as(ref)
        ratio = (out - ref).abs() / tol(ref)
        ratio = torch.where(torch.isfinite(out), ratio, torch.full_like(ratio, float("inf")))
        r = float(ratio.max())
        row, head, d = (int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        s = self.seq_of_row(row)
        msg = (f"{self.name}: {s.label} row {row - s.row0} (position {int(s.pos[row - s.row0])}) head {head} "
               f"element {d}: got {float(out[row, head, d])!r}, reference {float(ref[row, head, d])!r}, "
               f"error {r:.3g} x tolerance; element {d} carries the keys = {d} (mod {self.D})")
        return r, msg


MASK_MUTANTS = ("drop_newest", "drop_oldest", "admit_next", "admit_below", "drop_block_first", "drop_block_mid",
                "drop_block_last_full")
GATHER_MUTANTS = ("next_row", "head+1")
MUTANTS = MASK_MUTANTS + GATHER_MUTANTS


def _v_to_cache(v_block: torch.Tensor) -> torch.Tensor:
    """[nblk, 32 keys, Hkv, D] -> V cache [nblk, Hkv, D, 32] in its storage order (R.v_groups)."""
    inv = torch.argsort(R.v_slot_perm())                       # key held by each slot
    nb, _, h, D = v_block.shape
    g = v_block[:, inv].view(nb, 4, 8, h, D).permute(0, 3, 1, 4, 2)    # [nb, Hkv, 4, D, 8]
    return g.contiguous().view(nb, h, D, KV_BLOCK)


def _paged_pool(regime, ctx, Hkv, D, fp8, stretch, seed):
    """Pool with every sequence's keys, poison in every other slot; (kc, vc, bt, L, scales)."""
    L = 16 if fp8 else 48
    ks, vs = (0.5, 0.25) if fp8 else (1.0, 1.0)
    nbs = [(n + KV_BLOCK - 1) // KV_BLOCK for n in ctx]
    nblk = sum(nbs) + 1 + 3                                    # + padding target + unmapped blocks
    perm = torch.randperm(nblk, generator=torch.Generator().manual_seed(seed)).tolist()
    slot_keys = torch.arange(KV_BLOCK).repeat(nblk)
    K = _poison_rows(regime, slot_keys, Hkv, D, L).view(nblk, KV_BLOCK, Hkv, D).clone()
    V = torch.full((nblk, KV_BLOCK, Hkv, D), POISON_V, dtype=torch.float64)
    bt = torch.full((len(ctx), max(nbs) + 2), perm[nblk - 4], dtype=torch.int32)     # padding -> a poison block
    nxt = 0
    for i, n in enumerate(ctx):
        keys = torch.arange(nbs[i] * KV_BLOCK)
        k = _poison_rows(regime, keys, Hkv, D, L)
        v = torch.full((len(keys), Hkv, D), POISON_V, dtype=torch.float64)
        k[:n] = _key_rows(regime, keys[:n], Hkv, D, stretch, L, n, 4)
        v[:n] = tagged_v(keys[:n], Hkv, D, i)
        blocks = perm[nxt:nxt + nbs[i]]
        nxt += nbs[i]
        K[blocks] = k.view(nbs[i], KV_BLOCK, Hkv, D)
        V[blocks] = v.view(nbs[i], KV_BLOCK, Hkv, D)
        bt[i, :nbs[i]] = torch.tensor(blocks, dtype=torch.int32)
    dt = F8 if fp8 else torch.bfloat16
    kc = (K / ks).permute(0, 2, 1, 3).contiguous().float().to(dt)
    vc = _v_to_cache(V / vs).float().to(dt)
    return kc, vc, bt, ks, vs


DECODE_CTX = (1, 31, 32, 33, 64, 65, 129, 517, 900, 1025)
DECODE_AXES = {"regime": ["codebook", "levels"], "G": [1, 2, 4, 8, 16], "part_blocks": [4, 1000, -1, -3, -7],
               "window": [0, 1, 33, 100], "fp8": [False, True]}
PREFILL_SEQS = ((1, 1), (17, 17), (33, 33), (64, 64), (65, 200), (70, 300), (129, 450), (300, 300))
PREFILL_AXES = {"regime": ["codebook", "levels"], "G": [1, 2, 4, 8], "window": [0, 1, 40, 100], "fp8": [False, True]}
ENCODER_LENS = (1, 5, 31, 32, 33, 64, 130, 256, 300)
ENCODER_AXES = {"regime": ["codebook", "levels"], "D": [32, 64]}


def case_id(p: dict) -> str:
    return "-".join(f"{k}={v}" for k, v in p.items())


DECODE_PARAMS = pairwise(DECODE_AXES)
PREFILL_PARAMS = pairwise(PREFILL_AXES)
ENCODER_PARAMS = pairwise(ENCODER_AXES)


@functools.lru_cache(maxsize=None)
def decode_case(regime: str, G: int, window: int, fp8: bool, reps: int = 3) -> Case:
    """DECODE_CTX repeated ``reps`` times (the repeats share their physical blocks; 3 -> 30 rows,
    4 -> 40 rows: the nontemporal instantiation), Hkv = 2, D = 128."""
    Hkv, D = 2, 128
    Hq = Hkv * G
    kc, vc, bt, ks, vs = _paged_pool(regime, list(DECODE_CTX), Hkv, D, fp8, KV_BLOCK, seed=7)
    ctx = list(DECODE_CTX) * reps
    bt = bt.repeat(reps, 1).contiguous()
    q = torch.zeros(len(ctx), Hq, D, dtype=torch.float64)
    seqs = []
    for b, n in enumerate(ctx):
        for h in range(Hq):
            q[b, h] = _query(regime, 3 * (b // len(DECODE_CTX)) + b + h, h, G, h // G, n - 1, window, D,
                             flat=h == (b % 2) * G)
        seqs.append(Seq(row0=b, m=1, n=n, pos=torch.tensor([n - 1]), table_row=b, label=f"sequence {b} (ctx {n})"))
    name = f"decode[{regime} G={G} window={window} {'fp8' if fp8 else 'bf16'} B={len(ctx)}]"
    return Case("decode", name, regime, D, Hq, Hkv, window, ks, vs, q=q.bfloat16(), kc=kc, vc=vc, bt=bt, ctx=ctx,
                seqs=seqs)


@functools.lru_cache(maxsize=None)
def prefill_case(regime: str, G: int, window: int, fp8: bool) -> Case:
    Hkv, D = 2, 128
    Hq = Hkv * G
    ctx = [c for _, c in PREFILL_SEQS]
    kc, vc, bt, ks, vs = _paged_pool(regime, ctx, Hkv, D, fp8, 64, seed=11)
    cu = [0]
    for m, _ in PREFILL_SEQS:
        cu.append(cu[-1] + m)
    q = torch.zeros(cu[-1], Hq, D, dtype=torch.float64)
    seqs = []
    for i, (m, n) in enumerate(PREFILL_SEQS):
        pos = torch.arange(m) + (n - m)
        for r in range(m):
            for h in range(Hq):
                idx = r + h if regime == "codebook" else h + r // 16
                q[cu[i] + r, h] = _query(regime, idx, h, G, h // G, int(pos[r]), window, D, flat=h == (r % 2) * G)
        seqs.append(Seq(row0=cu[i], m=m, n=n, pos=pos, table_row=i, label=f"sequence {i} (q_len {m}, ctx {n})"))
    name = f"prefill[{regime} G={G} window={window} {'fp8' if fp8 else 'bf16'}]"
    return Case("prefill", name, regime, D, Hq, Hkv, window, ks, vs, q=q.bfloat16(), kc=kc, vc=vc, bt=bt, ctx=ctx,
                cu=cu, seqs=seqs)


@functools.lru_cache(maxsize=None)
def encoder_case(regime: str, D: int) -> Case:
    """ENCODER_LENS packed with a 2-token poison sequence before, between and after them."""
    H, L = 4, 48
    lens = [2]
    for n in ENCODER_LENS:
        lens += [n, 2]
    cu = [0]
    for n in lens:
        cu.append(cu[-1] + n)
    x = torch.zeros(cu[-1], 3, H, D, dtype=torch.float64)
    seqs = []
    for i, n in enumerate(lens):
        a = cu[i]
        if i % 2 == 0:       # poison: continues the numbering of the sequence before it (or precedes key 0)
            keys = torch.arange(2) + (lens[i - 1] if i else -2)
            x[a:a + n, 1] = _poison_rows(regime, keys, H, D, L)
            x[a:a + n, 2] = POISON_V
            x[a:a + n, 0] = x[a:a + n, 1] * (8.0 / D if regime == "codebook" else 0.0)
            label = f"poison sequence {i}"
        else:
            keys = torch.arange(n)
            x[a:a + n, 1] = _key_rows(regime, keys, H, D, KV_BLOCK, L, n, 1)
            x[a:a + n, 2] = tagged_v(keys, H, D)
            names = ("own", "key0", "last", "past_end", "mid_block", "zero")
            for r in range(n):
                for h in range(H):
                    if regime == "levels":
                        x[a + r, 0, h, (r + h) % NPROF] = 8.0
                        continue
                    t = {"own": r, "key0": 0, "last": n - 1, "past_end": n, "mid_block": (r // 64) * 32 + 13,
                         "zero": None}[names[(r + h) % len(names)]]
                    if t is not None:
                        x[a + r, 0, h] = (64.0 / D) * hadamard(D)[(t + 17 * h) % D]
            label = f"sequence {i} (len {n})"
        seqs.append(Seq(row0=a, m=n, n=n, pos=torch.full((n,), n - 1), beg=a, label=label, poison=i % 2 == 0))
    qkv = x.bfloat16().view(cu[-1], 3 * H * D)
    assert torch.equal(qkv.double().view_as(x), x)
    return Case("encoder", f"encoder[{regime} D={D}]", regime, D, H, H, qkv=qkv, q=qkv.view(cu[-1], 3, H, D)[:, 0],
                cu=cu, seqs=seqs)
