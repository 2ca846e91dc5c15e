"""In-flight batching on the host (pgmi/serve.py): the scheduler driven by a stub engine, and the slot step's rule
restated in numpy against a scalar transcription of DESIGN.md sec.1(i)'s text.  No GPU."""
import numpy as np
import pytest

from pgmi.serve import PARK_ID, SENTINEL, Scheduler, slot_finish_np


# ---------------------------------------------------------------- a stub engine: the slot state machine on the host
class StubEngine:
    """S slots that run scripted token streams: request r produces script[r][0] at its prefill and script[r][k]
    at its k-th step, through slot_finish_np (SENTINEL in a script: a step without a finite logit)."""

    def __init__(self, scripts, lens, budgets, S, n_steps, eos, pad, kv_max=1 << 20):
        self.scripts, self.lens, self.budgets = scripts, lens, budgets
        self.S, self.n_steps, self.eos, self.pad, self.kv_max = S, n_steps, eos, pad, kv_max
        self.live = np.zeros(S, np.int64)
        self.left = np.zeros(S, np.int64)
        self.kv = np.zeros(S, np.int64)
        self.pos = np.zeros(S, np.int64)
        self.req = [None] * S       # request whose script the slot reads
        self.k = [0] * S            # tokens of it taken so far
        self.pending = {}
        self.admits = []            # (slots, requests) of every admit call
        self.steps = 0

    def admit(self, slots, reqs):
        assert len(slots) == len(reqs) and len(set(slots)) == len(slots)
        self.admits.append((list(slots), list(reqs)))
        for s, r in zip(slots, reqs):
            assert self.live[s] != 1, "admission into a running slot"
            first = self.scripts[r][0]
            live = first != self.eos and self.budgets[r] > 1
            self.live[s], self.left[s] = int(live), self.budgets[r] - 1
            self.kv[s], self.pos[s] = (self.lens[r], self.lens[r] + 1) if live else (0, 0)
            self.req[s], self.k[s] = r, 1
            self.pending[s] = first

    def step(self):
        rec = []
        for _ in range(self.n_steps):
            tok = np.array([self.scripts[self.req[s]][self.k[s]] if self.live[s] == 1 else 12345
                            for s in range(self.S)], np.int64)
            for s in range(self.S):
                self.k[s] += int(self.live[s] == 1)
            out, _, self.live, self.left, self.kv, self.pos = slot_finish_np(
                tok, self.live, self.left, self.kv, self.pos, self.eos, self.pad, self.kv_max)
            rec.append(out.tolist())
            self.steps += 1
        first, self.pending = self.pending, {}
        return rec, first

    def state(self):
        return self.live.tolist(), self.left.tolist()


def serve_stub(scripts, budgets, S, n_steps=4, admit_group=8, eos=-1, pad=-7):
    lens = [10 + r for r in range(len(scripts))]
    eng = StubEngine(scripts, lens, budgets, S, n_steps, eos, pad)
    sch = Scheduler(eng, budgets, S, admit_group)
    toks, codes = sch.run()
    return toks, codes, eng, sch


def stream(r, n=40):
    return [100 * (r + 1) + k for k in range(n)]


def test_budget_harvest_and_slot_reuse():
    budgets = [3, 9, 1, 5, 2, 6, 4]
    scripts = [stream(r) for r in range(len(budgets))]
    toks, codes, eng, sch = serve_stub(scripts, budgets, S=3, n_steps=4)
    for r, b in enumerate(budgets):
        assert toks[r] == scripts[r][:b], r
    assert codes == [0] * len(budgets)
    # admission order: the head of the queue into the free slots in ascending order
    assert eng.admits[0] == ([0, 1, 2], [0, 1, 2])
    # after the first launch slots 0 (budget 3) and 2 (budget 1) are free, slot 1 (budget 9) still runs
    assert eng.admits[1] == ([0, 2], [3, 4])
    served = [r for _, rq in eng.admits for r in rq]
    assert served == list(range(len(budgets)))
    assert sch.launches * 4 == eng.steps


def test_admit_group_splits_admissions():
    budgets = [2, 2, 2, 2, 2]
    scripts = [stream(r) for r in range(5)]
    _, _, eng, _ = serve_stub(scripts, budgets, S=4, admit_group=1)
    assert eng.admits[:4] == [([0], [0]), ([1], [1]), ([2], [2]), ([3], [3])]
    _, _, eng3, _ = serve_stub(scripts, budgets, S=4, admit_group=3)
    assert eng3.admits[:2] == [([0, 1, 2], [0, 1, 2]), ([3], [3])]


def test_eos_harvest_and_first_token_eos():
    eos = 7
    scripts = [[1, 2, eos, 50, 51, 52],        # stops at its third token
               [eos, 60, 61, 62],              # the prefill's token is the stop token: parked by the admission
               [3, 4, 5, 6, 8, 9, 10, 11],     # never stops: runs to its budget
               [9, eos, 70, 71]]               # admitted into a freed slot, stops at its first step
    budgets = [6, 4, 8, 4]
    toks, codes, eng, _ = serve_stub(scripts, budgets, S=2, n_steps=2, eos=eos, pad=eos)
    assert toks == [[1, 2, eos], [eos], [3, 4, 5, 6, 8, 9, 10, 11], [9, eos]]
    assert codes == [0, 0, 0, 0]
    assert eng.admits[0] == ([0, 1], [0, 1])
    assert eng.admits[1] == ([0, 1], [2, 3])   # both parked within the first launch


def test_pad_equal_to_a_token_is_not_a_stop():
    # pad is a legal id that the request also produces: the count comes from `left`, not from comparing with pad
    scripts = [[5, -7, -7, 6, 8], [1, 2, 3]]
    toks, _, _, _ = serve_stub(scripts, [5, 2], S=2, n_steps=8, pad=-7)
    assert toks == [[5, -7, -7, 6, 8], [1, 2]]


def test_no_finite_logit_code():
    scripts = [[1, 2, SENTINEL, 9, 9], [4, 5, 6, 7]]
    toks, codes, _, _ = serve_stub(scripts, [5, 4], S=2, n_steps=3)
    assert toks == [[1, 2], [4, 5, 6, 7]]
    assert codes == [-1, 0]


def test_empty_queue_and_more_slots_than_requests():
    toks, codes, eng, sch = serve_stub([], [], S=4)
    assert toks == [] and codes == [] and eng.steps == 0 and sch.launches == 0
    scripts = [stream(0), stream(1)]
    toks, codes, eng, _ = serve_stub(scripts, [3, 5], S=8, n_steps=4)
    assert toks == [scripts[0][:3], scripts[1][:5]] and codes == [0, 0]
    assert eng.admits == [([0, 1], [0, 1])]
    assert eng.steps == 4       # one launch: both park inside it


def test_scheduler_argument_checks():
    with pytest.raises(ValueError):
        Scheduler(None, [1], 0)
    with pytest.raises(ValueError):
        Scheduler(None, [1], 2, admit_group=0)
    with pytest.raises(ValueError):
        Scheduler(None, [3, 0], 2)


# ---------------------------------------------------------------- the slot step's rule
def slot_finish_scalar(tok, live, left, kv, pos, eos, pad):
    """One slot, transcribed from DESIGN.md sec.1(i)."""
    if live != 1:
        return pad, PARK_ID, live, left, kv, pos
    if tok == SENTINEL:
        return pad, PARK_ID, -1, left, 0, 0
    left -= 1
    if tok != eos and left > 0:
        return tok, tok, 1, left, kv + 1, pos + 1
    return tok, PARK_ID, 0, left, 0, 0


@pytest.mark.parametrize("eos", [-1, 3])
def test_slot_finish_rule_300_rows(eos):
    rng = np.random.default_rng(17)
    n = 300
    tok = rng.integers(0, 6, n)
    tok[rng.random(n) < 0.1] = SENTINEL
    live = rng.choice([1, 1, 1, 0, -1], n)
    left = np.where(live == 1, rng.integers(1, 5, n), rng.integers(0, 5, n))
    kv = np.where(live == 1, rng.integers(1, 500, n), 0)
    pos = np.where(live == 1, kv + 1, 0)
    got = slot_finish_np(tok, live, left, kv, pos, eos, -7)
    seen = set()
    for i in range(n):
        want = slot_finish_scalar(int(tok[i]), int(live[i]), int(left[i]), int(kv[i]), int(pos[i]), eos, -7)
        assert tuple(int(g[i]) for g in got) == want, (i, tok[i], live[i], left[i])
        seen.add((int(live[i]), want[2]))
    # every transition occurs among the 300 rows: runs on, parks, parks without a finite logit, stays parked
    assert {(1, 1), (1, 0), (1, -1), (0, 0), (-1, -1)} <= seen


def test_slot_finish_never_reaches_kv_max():
    out = slot_finish_np([5, 5], [1, 1], [9, 9], [14, 15], [15, 16], -1, -7, kv_max=16)
    assert out[2].tolist() == [1, 0] and out[4].tolist() == [15, 0]
