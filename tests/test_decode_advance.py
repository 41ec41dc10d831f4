"""The decode-advance kernels and their stop-string matcher against a plain model of the operation.

``decode_advance_kernel``, ``decode_advance_cb_kernel`` and ``stop_feed`` (csrc/kernels/
elementwise.hip) run once per generated token: they store the token, pick the KV slot the next step
writes and decide when a sequence stops.  The model below is written from the definition, with
lists and ``bytes`` only (nothing of runtime/stops.py or ops/kernels.py):

* the text of a slot is its tokens' bytes joined, minus ONE leading space when ``strip`` is set; a
  stop completes at the first token whose arrival makes the text contain a stop string;
* static step: every row records the token (while ``step < max_new``), advances position, context
  length and KV slot, and is marked done on a stop string (``keep = step + 1``) or a stop id; rows
  already done still advance but no longer feed the matcher;
* continuous step: a done slot changes nothing at all; any other records the token (while
  ``gen < cap``), counts it, finishes on its limit, a stop id or a stop string (``keep = gen``),
  and only a slot still running takes the new input id, position, context length and KV slot.

After every one of 16 steps the whole state of the CPU branches (everywhere) and of the kernels (on
the GPU, eager and replayed from a captured graph) must equal the model's exactly.
"""
from __future__ import annotations

import functools
import random

import pytest
import torch

from copilot_for_consensus_amd.ops import kernels as K
from copilot_for_consensus_amd.runtime.stops import StopStringMatcher

VOCAB = [b"", b"\n", b"\n\n", b".\n", b"\nThe", b"</", b"s>", b"<", b"/s", b">", b" a", b"b", b"x\n\n\ny",
         b"\n\n\n", b"ok", b" </s", b"> end", b"\n\n\n\n", b" ", b"  ", b"a", b"ab", b"aab", b"ba",
         b"abcdefghijklmnopqrstuvwxyz0123456789ABCDEFG", b" \n"]
STOP_SETS = [["</s>", "\n\n\n"],
             [" a", "\n\n\n"],
             ["a"],                                   # L = 1, H = 1
             ["aab", "ab", "\n\n"],                   # one stop is a suffix of another
             ["abaab", "ba"],                         # self-overlap
             ["  a"],
             ["z0123456789ABCDEFG\n", "abcdefghijklmnopqrstuvwxyz012345"]]    # L = 32, the maximum
# A stop of STOP_SETS[2] is one byte, and the first stop of STOP_SETS[6] needs the 43-byte token,
# which holds the second stop whole: neither set can complete a stop across two tokens.
CAN_STRADDLE = [True, True, False, True, True, True, False]
# ids that stop a row by themselves: "ok" alone, or three tokens that also complete a stop string
# of every set ("\n\n\n"; "aab" alone, after "ab" and after "  "; the 43-byte token)
STOP_IDS = {0: [], 1: [VOCAB.index(b"ok")],
            3: [VOCAB.index(b"\n\n\n"), VOCAB.index(b"aab"), VOCAB.index(VOCAB[24])]}
FILLER = [VOCAB.index(b) for b in (b"", b"b", b">", b"s>")]

KV_BS = 32
STEPS = 16
MAX_NEW = 12            # < STEPS: the last steps must not record their tokens
MAX_BLOCKS = 7          # positions reach 95 + 16: 4 blocks are used
GUARD_ROWS = 2          # rows after `tokens` in its buffer, which no step may write
START_POS = [0, 29, 30, 31, 61, 62, 63, 95]
LIMITS = [1, 5, 12, 40]
KEEP_ALL = 1 << 30


# ------------------------------------------------------------------------------------ the model

def tok_bytes(t: int) -> bytes:
    return VOCAB[t] if 0 <= t < len(VOCAB) else b""


def text_of(toks, strip: bool) -> bytes:
    b = b"".join(tok_bytes(t) for t in toks)
    return b[1:] if strip and b[:1] == b" " else b


def first_stop(toks, stops, strip: bool):
    """Index of the first token with which the text contains a stop, or None."""
    for i in range(len(toks)):
        t = text_of(toks[:i + 1], strip)
        if any(s in t for s in stops):
            return i
    return None


class TextRule:
    """A slot's matcher state is ``raw``, every byte its tokens brought so far."""

    def __init__(self, stops, strip: bool):
        self.stops = [s.encode() for s in stops]
        self.strip = strip
        self.H = max(1, max(len(s) for s in self.stops) - 1)

    def text(self, raw: bytes) -> bytes:
        return raw[1:] if self.strip and raw[:1] == b" " else raw

    def hit(self, raw: bytes) -> bool:
        t = self.text(raw)
        return any(s in t for s in self.stops)

    def straddles(self, before: bytes, raw: bytes) -> bool:
        """The stop that ``raw`` completes lies in no token alone: it began before the last one."""
        new = self.text(raw)[len(self.text(before)):]
        return not any(s in new for s in self.stops)

    def window(self, raw: bytes):
        """(wlen, the last H bytes of the text); wlen -1 while no token brought a byte."""
        t = self.text(raw)
        return (-1 if not raw else min(len(t), self.H)), t[-self.H:]


def slot_of(block_row, pos: int) -> int:
    return block_row[pos // KV_BS] * KV_BS + pos % KV_BS


class Model:
    """Both kernels' state as lists; ``case`` holds the initial values (see make_case)."""

    def __init__(self, case):
        c = case
        self.kind, self.B = c["kind"], c["B"]
        self.rule = TextRule(c["stops"], c["strip"]) if c["stops"] else None
        self.stop_ids = set(c["stop_ids"])
        self.block_tables = c["block_tables"]
        self.tokens = [list(r) for r in c["tokens"]]            # B + GUARD_ROWS rows
        self.width = len(self.tokens[0])
        self.step = 0
        self.gen, self.limit = list(c["gen"]), list(c["limit"])
        self.input_ids, self.positions = list(c["input_ids"]), list(c["positions"])
        self.ctx_lens = [p + 1 for p in self.positions]
        self.slots = [slot_of(self.block_tables[b], self.positions[b]) for b in range(self.B)]
        self.done, self.keep = list(c["done"]), list(c["keep"])
        self.raw = list(c["raw"])                 # bytes, or (wlen, window) of a slot preset done
        # what the fixture exercises, from the model alone
        self.string_stop = {}                     # row -> (step, straddles, a stop id at the same step)

    def _feed(self, b: int, t: int) -> bool:
        before = self.raw[b]
        self.raw[b] = before + tok_bytes(t)
        if not self.rule.hit(self.raw[b]):
            return False
        self.string_stop[b] = (self.step, self.rule.straddles(before, self.raw[b]), t in self.stop_ids)
        return True

    def _move(self, b: int, t: int) -> None:
        self.input_ids[b] = t
        self.positions[b] += 1
        self.ctx_lens[b] = self.positions[b] + 1
        self.slots[b] = slot_of(self.block_tables[b], self.positions[b])

    def advance(self, nxt) -> None:
        for b in range(self.B):
            t = nxt[b]
            if self.kind == "static":
                if self.step < self.width:
                    self.tokens[b][self.step] = t
                self._move(b, t)
                if self.rule and not self.done[b] and self._feed(b, t):
                    self.done[b] = 1
                    self.keep[b] = self.step + 1
                if t in self.stop_ids:
                    self.done[b] = 1
            elif not self.done[b]:
                if self.gen[b] < self.width:
                    self.tokens[b][self.gen[b]] = t
                self.gen[b] += 1
                d = self.gen[b] >= self.limit[b] or t in self.stop_ids
                if self.rule and self._feed(b, t):
                    d = True
                    self.keep[b] = self.gen[b]
                self.done[b] = int(d)
                if not d:
                    self._move(b, t)
        self.step += 1

    def window(self, b: int):
        r = self.raw[b]
        return r if isinstance(r, tuple) else self.rule.window(r)

    def snapshot(self) -> dict:
        s = dict(tokens=[list(r) for r in self.tokens], input_ids=list(self.input_ids),
                 positions=list(self.positions), ctx_lens=list(self.ctx_lens), slots=list(self.slots),
                 done=list(self.done))
        if self.kind == "static":
            s["step"] = [self.step]
        else:
            s["gen"] = list(self.gen)
        if self.rule:
            w = [self.window(b) for b in range(self.B)]
            s["keep"] = list(self.keep)
            s["wlen"] = [x[0] for x in w]
            s["win"] = [x[1] for x in w]
        return s


def make_case(kind: str, B: int, n_stop: int, set_idx, strip: bool) -> dict:
    """Initial state and the 16 sampled tokens of every row, as plain lists.

    Rows start at positions around the KV block boundaries, in blocks that are a random permutation
    of a pool.  Tokens are uniform over the toy vocabulary; every fourth row draws three of four
    from pieces of no stop, so that rows run to the end under every stop set.  With a stop set, a
    third of the rows already hold one or two tokens' text (the engines feed the prefill's token on
    the host); such a row is done from the start when that text holds a stop.  Continuous: a
    quarter of the slots are preset done, with arbitrary counters and windows."""
    rng = random.Random(f"{kind}/{B}/{n_stop}/{set_idx}/{int(strip)}")
    stops = STOP_SETS[set_idx] if set_idx is not None else None
    rule = TextRule(stops, strip) if stops else None
    pool = list(range(B * MAX_BLOCKS))
    rng.shuffle(pool)
    c = dict(kind=kind, B=B, stops=stops, strip=strip, stop_ids=STOP_IDS[n_stop],
             block_tables=[pool[b * MAX_BLOCKS:(b + 1) * MAX_BLOCKS] for b in range(B)],
             tokens=[[-1] * MAX_NEW for _ in range(B + GUARD_ROWS)],
             positions=[rng.choice(START_POS) for _ in range(B)],
             input_ids=[rng.randrange(len(VOCAB)) for _ in range(B)],
             gen=[0] * B, limit=[0] * B, done=[0] * B, keep=[KEEP_ALL] * B, raw=[b""] * B, preset=[])
    c["stream"] = [[rng.choice(FILLER) if b % 4 == 3 and rng.random() < 0.75 else rng.randrange(len(VOCAB))
                    for b in range(B)] for _ in range(STEPS)]
    for b in range(B):
        if kind == "cb":
            c["gen"][b] = rng.choice([0, 1, 3])
            c["limit"][b] = rng.choice(LIMITS)
            if b % 4 == 2:
                c["done"][b] = 1
                c["gen"][b] = rng.randrange(16)
                c["tokens"][b] = [rng.randrange(len(VOCAB)) for _ in range(MAX_NEW)]
                if rule:
                    c["keep"][b] = rng.randrange(1, MAX_NEW + 1)
                    c["raw"][b] = (rng.randrange(-1, rule.H + 1), bytes(rng.randrange(256) for _ in range(rule.H)))
                    c["preset"].append(b)
                continue
        if rule and rng.random() < 1 / 3:
            prefix = [rng.randrange(len(VOCAB)) for _ in range(rng.choice([1, 2]))]
            c["raw"][b] = b"".join(tok_bytes(t) for t in prefix)
            if rule.hit(c["raw"][b]):
                c["done"][b] = 1
                c["keep"][b] = len(prefix)
    return c


@functools.lru_cache(maxsize=None)
def model_run(kind: str, B: int, n_stop: int, set_idx, strip: bool):
    """(case, the model's state after each step, the model at the end): computed once, shared by
    the CPU and the GPU tests, never changed."""
    case = make_case(kind, B, n_stop, set_idx, strip)
    m = Model(case)
    snaps = []
    for s in range(STEPS):
        m.advance(case["stream"][s])
        snaps.append(m.snapshot())
    return case, snaps, m


def case_list(Bs):
    """Every B without stop strings under 0, 1 and 3 stop ids, and with each stop set under both
    strip values (3 stop ids when stripping; none or one otherwise)."""
    out = []
    for B in Bs:
        out += [(B, n, None, False) for n in (0, 1, 3)]
        out += [(B, 3 if strip else si % 2, si, strip) for si in range(len(STOP_SETS))
                for strip in (False, True)]
    return out


def case_id(c) -> str:
    B, n, si, strip = c
    return f"B{B}-ids{n}-" + ("nostr" if si is None else f"set{si}-strip{int(strip)}")


# ------------------------------------------------------------------- the code under test, driven

@functools.lru_cache(maxsize=None)
def matcher(set_idx: int, strip: bool) -> StopStringMatcher:
    return StopStringMatcher(lambda i: VOCAB[i], len(VOCAB), STOP_SETS[set_idx], strip_leading_space=strip)


class Driven:
    """The tensors of one case on ``device`` and one call of the wrapper per step."""

    def __init__(self, case, set_idx, device):
        c = self.case = case
        B = self.B = c["B"]
        self.kind = c["kind"]
        t = lambda x: torch.tensor(x, dtype=torch.int32, device=device)     # noqa: E731
        self.buf = t(c["tokens"])
        self.tokens = self.buf[:B]              # the leading rows of a larger buffer
        self.step = t([0])
        self.gen, self.limit = t(c["gen"]), t(c["limit"])
        self.input_ids, self.positions = t(c["input_ids"]), t(c["positions"])
        self.ctx_lens = t([p + 1 for p in c["positions"]])
        self.block_tables = t(c["block_tables"])
        self.slots = t([slot_of(c["block_tables"][b], c["positions"][b]) for b in range(B)])
        self.done = t(c["done"])
        self.stop_ids = t(c["stop_ids"])
        self.next_ids = torch.zeros(B, dtype=torch.int32, device=device)
        self.stream = t(c["stream"])
        self.state = None
        if c["stops"]:
            m = matcher(set_idx, c["strip"])
            st = self.state = m.new_state(B, device)
            # rows that hold text already: installed as the engines do after the prefill's token
            rule = TextRule(c["stops"], c["strip"])
            rows = [b for b in range(B) if isinstance(c["raw"][b], bytes) and c["raw"][b]]
            if rows:
                wins = [rule.window(c["raw"][b]) for b in rows]
                st.set_slots(rows, [(w[:max(n, 0)], n < 0) for n, w in wins], [c["keep"][b] for b in rows])
            if c["preset"]:
                idx = torch.tensor(c["preset"], dtype=torch.long, device=device)
                st.wlen[idx] = t([c["raw"][b][0] for b in c["preset"]])
                st.keep[idx] = t([c["keep"][b] for b in c["preset"]])
                st.win[idx] = torch.tensor([list(c["raw"][b][1]) for b in c["preset"]], dtype=torch.uint8,
                                           device=device)

    def call(self) -> None:
        if self.kind == "static":
            K.decode_advance(self.next_ids, self.tokens, self.step, self.input_ids, self.positions, self.ctx_lens,
                             self.slots, self.block_tables, self.done, self.stop_ids, self.state)
        else:
            K.decode_advance_cb(self.next_ids, self.tokens, self.gen, self.limit, self.input_ids, self.positions,
                                self.ctx_lens, self.slots, self.block_tables, self.done, self.stop_ids, self.state)

    def read(self) -> dict:
        s = dict(tokens=self.buf, input_ids=self.input_ids, positions=self.positions, ctx_lens=self.ctx_lens,
                 slots=self.slots, done=self.done)
        s["step" if self.kind == "static" else "gen"] = self.step if self.kind == "static" else self.gen
        if self.state is not None:
            s.update(keep=self.state.keep, wlen=self.state.wlen, win=self.state.win)
        s = {k: v.cpu().tolist() for k, v in s.items()}
        if self.state is not None:
            # bytes past wlen are unspecified, except in a slot preset done: nothing of it may change
            frozen = set(self.case["preset"])
            s["win"] = [bytes(w if b in frozen else w[:max(n, 0)])
                        for b, (w, n) in enumerate(zip(s["win"], s["wlen"]))]
        return s


def assert_same(got: dict, want: dict, where: str) -> None:
    assert got.keys() == want.keys()
    for k in want:
        if got[k] != want[k]:
            bad = [i for i, (g, w) in enumerate(zip(got[k], want[k])) if g != w]
            i = bad[0]
            raise AssertionError(f"{where}: {k} differs in {len(bad)} rows, first row {i}: "
                                 f"got {got[k][i]!r}, model {want[k][i]!r}")


def run_against_model(kind, params, device, graph=False):
    B, n_stop, set_idx, strip = params
    case, snaps, _ = model_run(kind, B, n_stop, set_idx, strip)
    d = Driven(case, set_idx, device)
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            d.call()
    for s in range(STEPS):
        d.next_ids.copy_(d.stream[s])
        g.replay() if graph else d.call()
        assert_same(d.read(), snaps[s], f"{kind} {case_id(params)} {'replay' if graph else 'step'} {s}")


# ------------------------------------------------------------------ host matcher vs the text rule

@pytest.mark.parametrize("strip", [False, True], ids=["keep-space", "strip-space"])
@pytest.mark.parametrize("set_idx", range(len(STOP_SETS)))
def test_host_matcher_equals_text_rule(set_idx, strip):
    m = matcher(set_idx, strip)
    stops = [s.encode() for s in STOP_SETS[set_idx]]
    rng = random.Random(1000 + 2 * set_idx + strip)
    hits = 0
    for _ in range(2000):
        ids = [rng.randrange(len(VOCAB)) for _ in range(rng.randrange(1, 12))]
        want = first_stop(ids, stops, strip)
        assert m.match_tokens(ids) == want, (ids, [VOCAB[i] for i in ids])
        hits += want is not None
    assert 40 <= hits <= 1900, hits         # the streams stop, and run on, often enough to matter


def test_leading_space_that_decode_drops_is_no_stop():
    ix = VOCAB.index
    m = matcher(1, True)                    # stops " a", "\n\n\n"
    assert text_of([ix(b" a")], True) == b"a"
    assert m.match_tokens([ix(b" a")]) is None
    assert m.match_tokens([ix(b" a"), ix(b" a")]) == 1          # "a a": the second space stays
    assert matcher(1, False).match_tokens([ix(b" a")]) == 0
    # a stop inside the first token's bytes only once the space is gone is still a stop
    assert matcher(2, True).match_tokens([ix(b" a")]) == 0


def test_leading_space_is_dropped_once():
    ix = VOCAB.index
    m = matcher(5, True)                    # stop "  a"
    ids = [ix(b" "), ix(b"  "), ix(b""), ix(b"a")]
    assert text_of(ids, True) == b"  a"
    assert m.match_tokens(ids) == 3
    assert m.match_tokens([ix(b""), ix(b" "), ix(b"  "), ix(b"a")]) == 3    # empty tokens first: still fresh
    assert m.match_tokens([ix(b" "), ix(b" a")]) is None                    # " a": one space short
    st, hit = m.feed(m.initial(), ix(b" "))
    assert st == (b"", False) and not hit   # nothing remains of the token, yet the text has begun


def test_stop_longer_than_the_window_is_refused():
    StopStringMatcher(lambda i: VOCAB[i], len(VOCAB), ["x" * 32])
    with pytest.raises(ValueError):
        StopStringMatcher(lambda i: VOCAB[i], len(VOCAB), ["</s>", "x" * 33])


def test_tables_cover_the_models_vocabulary():
    """A model whose embedding is padded past the tokenizer's vocabulary samples ids the tokenizer
    does not know: the tables the kernels index need a (zero-length) row for each."""
    class Tok:
        vocab_size = 20
        strips_leading_space = True

        def token_bytes(self, i):
            return VOCAB[i]

    m = StopStringMatcher.for_tokenizer(Tok(), [" a", "\n\n\n"])
    st = m.new_state(2, "cpu", vocab_size=32)
    a = st.kernel_args()
    for k in ("head", "tail", "tlen", "contains"):
        assert a[k].shape[0] == 32, k
        assert not a[k][20:].any(), k
    i32 = lambda x: torch.tensor(x, dtype=torch.int32)      # noqa: E731
    tokens, step, done = torch.full((2, 4), -1, dtype=torch.int32), i32([0]), i32([0, 0])
    ids, pos, ctx, slots, bt = i32([0, 0]), i32([0, 0]), i32([1, 1]), i32([0, 0]), i32([[3], [5]])
    for want_wlen, nxt in (([-1, 1], [25, 11]), ([1, 1], [10, 25]), ([1, 1], [31, 25])):
        K.decode_advance(i32(nxt), tokens, step, ids, pos, ctx, slots, bt, done, i32([]), st)
        assert st.wlen.tolist() == want_wlen and done.tolist() == [0, 0]
    assert bytes(st.win[:, 0].tolist()) == b"ab"            # " a" came first in row 0: its space is gone
    assert m.match_tokens([25, 10]) is None and m.match_tokens([25, 13, 31]) == 1


# ------------------------------------------------------------- what the fixtures exercise (model)

@pytest.mark.parametrize("strip", [False, True], ids=["keep-space", "strip-space"])
@pytest.mark.parametrize("set_idx", range(len(STOP_SETS)))
def test_static_fixture_stops_and_runs_on(set_idx, strip):
    """Counted on the model alone, for the B = 1024 case of every stop set."""
    n_stop = 3 if strip else set_idx % 2
    case, _, m = model_run("static", 1024, n_stop, set_idx, strip)
    assert len(m.string_stop) >= 10
    assert sum(not d for d in m.done) >= 10                 # rows that run through all 16 steps
    if CAN_STRADDLE[set_idx]:
        assert any(straddles for _, straddles, _ in m.string_stop.values())
    if n_stop == 3:
        assert any(with_id for _, _, with_id in m.string_stop.values())
    assert any(step >= MAX_NEW for step, _, _ in m.string_stop.values())    # keep > max_new happens
    started = [b for b in range(1024) if case["raw"][b]]
    assert len(started) >= 100
    if not (set_idx == 5 and strip):        # "  a" after the dropped space takes three tokens, not two
        assert any(case["done"][b] for b in started)
    # rows cross 31 -> 32 and 63 -> 64 inside the run
    assert {29, 30, 31, 61, 62, 63} <= set(case["positions"])


@pytest.mark.parametrize("params", case_list([300]), ids=case_id)
def test_continuous_fixture_finishes_rows_at_different_steps(params):
    case, snaps, m = model_run("cb", *params)
    B = params[0]
    preset = [b for b in range(B) if case["done"][b] and b % 4 == 2]
    assert len(preset) == B // 4
    fin = {}
    for s, snap in enumerate(snaps):
        for b in range(B):
            if snap["done"][b] and not case["done"][b]:
                fin.setdefault(b, s)
    assert len(set(fin.values())) >= 7                      # the limits 1, 5, 12 and the stops in between
    assert not all(m.done)                                  # limit 40 and nothing stopped it
    assert sum(g > MAX_NEW for g in m.gen) >= 10            # counted past the capacity of `tokens`
    if params[2] is not None:
        # 225 running slots, a quarter of them with 16 tokens to go: fewer stops than at B = 1024
        assert len(m.string_stop) >= 5


# ----------------------------------------------------------------- the CPU branches vs the model

CPU_STATIC = case_list([1, 64, 65, 1024])
CPU_CB = case_list([1, 65, 300])


@pytest.mark.parametrize("params", CPU_STATIC, ids=case_id)
def test_decode_advance_cpu_equals_model(params):
    run_against_model("static", params, "cpu")


@pytest.mark.parametrize("params", CPU_CB, ids=case_id)
def test_decode_advance_cb_cpu_equals_model(params):
    run_against_model("cb", params, "cpu")


# ------------------------------------------------------------------------ the kernels vs the model

@pytest.mark.gpu
@pytest.mark.parametrize("params", case_list([1, 64, 65, 1024]), ids=case_id)
def test_decode_advance_kernel_equals_model(params):
    run_against_model("static", params, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("params", case_list([1, 65, 300]), ids=case_id)
def test_decode_advance_cb_kernel_equals_model(params):
    run_against_model("cb", params, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("set_idx", [None, 0])
def test_decode_advance_refuses_more_than_one_workgroup(set_idx):
    """B = 1025: the launcher's return code, raised by the wrapper before anything is written."""
    d = Driven(make_case("static", 1025, 1, set_idx, True), set_idx, "cuda")
    d.next_ids.copy_(d.stream[0])
    before = d.read()
    with pytest.raises(RuntimeError):
        d.call()
    torch.cuda.synchronize()
    assert_same(d.read(), before, "B = 1025")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,params", [("static", (65, 3, 1, True)), ("cb", (300, 3, 5, True)),
                                         ("static", (1024, 1, None, False))],
                         ids=["static-B65-set1", "cb-B300-set5", "static-B1024-nostr"])
def test_decode_advance_replayed_from_a_graph(kind, params):
    """One captured launch, ``next_ids`` refilled before each replay: the same 16 states as the
    eager run (both are compared with the model's)."""
    run_against_model(kind, params, "cuda")
    run_against_model(kind, params, "cuda", graph=True)
