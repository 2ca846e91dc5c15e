"""In-flight batching, host side: the scheduler of a serving loop, and a slot step's rule restated in numpy.

A batch of S *slots* (KV row b of one cache) in which a row that stops *parks* and the next request takes its place
while the others keep running -- DESIGN.md sec.1(i) has the state machine.  This module is the part that needs no
GPU: no torch, no library call.  The device side (a slot step's last kernel, the admission kernel, the prefill into
a named KV row) is not in the library yet; the scheduler drives any object with three
methods, and the CPU tests drive it with a stub that runs the rule below:

    admit(slots, requests)  prefill requests[i] (an index into the request list) into KV slot slots[i] and admit it
    step()                  run one launch of the slot steps; returns (record, first) -- record[t][s] the token slot
                            s recorded at step t of the launch, first[s] the prefill token of every slot admitted
                            since the previous step() (a dict)
    state()                 (live, left) per slot after the launch: live 1 running, 0 parked, -1 parked because its
                            logits had no finite maximum; left the tokens the slot may still produce

A request's tokens are its first token, then what its slot recorded until it parked.  How many that is comes from the
driver's own count (budget - left), never from comparing a recorded value with pad: pad may be a legal token id.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

SENTINEL = 0x7FFFFFFF  # the argmax reduction's index when no logit was finite (k_argmax_finish's start value)
PARK_ID = 0            # what a parked slot feeds itself: row 0 of the embedding


def slot_finish_np(token, live, left, kv_len, position, eos: int, pad: int, kv_max: int = 1 << 30):
    """The rule a slot step's last kernel applies, for arrays of slots (numpy): token is each slot's argmax
    (SENTINEL: no finite logit).
    Returns (recorded, ids, live, left, kv_len, position) after the step; ids is what the slot feeds back
    (the token, or PARK_ID once parked).  eos -1: no stop token."""
    import numpy as np
    token = np.asarray(token, dtype=np.int64)
    live = np.asarray(live, dtype=np.int64)
    left = np.asarray(left, dtype=np.int64)
    kv_len = np.asarray(kv_len, dtype=np.int64)
    position = np.asarray(position, dtype=np.int64)
    running = live == 1
    nan = running & (token == SENTINEL)
    took = running & ~nan
    left2 = np.where(took, left - 1, left)
    go = took & (token != eos) & (left2 > 0) & (kv_len + 1 < kv_max)
    live2 = np.where(nan, -1, np.where(took & ~go, 0, live))
    recorded = np.where(took, token, pad)
    ids = np.where(go, token, PARK_ID)
    kv2 = np.where(go, kv_len + 1, np.where(running, 0, kv_len))
    pos2 = np.where(go, position + 1, np.where(running, 0, position))
    return recorded, ids, live2, left2, kv2, pos2


class Scheduler:
    """Serves `budgets[r]` tokens for request r = 0 .. len(budgets) - 1 through `n_slots` slots of `driver`.

    Free slots are filled in ascending order from the head of the queue, at most `admit_group` requests per admit()
    call; then one step() launch, one state() read, and the slots that parked are harvested and become free."""

    def __init__(self, driver, budgets: Sequence[int], n_slots: int, admit_group: int = 8):
        if n_slots < 1:
            raise ValueError("serve: at least one slot")
        if admit_group < 1:
            raise ValueError("serve: admit_group must be >= 1")
        for b in budgets:
            if int(b) < 1:
                raise ValueError("serve: every request needs max_new_tokens >= 1")
        self.driver = driver
        self.budgets = [int(b) for b in budgets]
        self.n_slots = int(n_slots)
        self.admit_group = int(admit_group)
        self.queue: List[int] = list(range(len(self.budgets)))
        self.holder: List[Optional[int]] = [None] * self.n_slots  # the request each slot runs
        self.tokens: List[List[int]] = [[] for _ in self.budgets]
        self.codes: List[int] = [0] * len(self.budgets)
        self.launches = 0
        self.admissions = 0

    def _admit(self) -> None:
        free = [s for s in range(self.n_slots) if self.holder[s] is None]
        while free and self.queue:
            g = min(len(free), len(self.queue), self.admit_group)
            slots, reqs = free[:g], self.queue[:g]
            del free[:g], self.queue[:g]
            for s, r in zip(slots, reqs):
                self.holder[s] = r
            self.driver.admit(slots, reqs)
            self.admissions += 1

    def _harvest(self, record, first: Dict[int, int], live, left) -> None:
        for s, r in enumerate(self.holder):
            if r is None:
                continue
            out = self.tokens[r]
            if s in first:
                out.append(int(first[s]))
            # the device's count of what the request has produced so far, its first token included
            total = self.budgets[r] - int(left[s])
            for row in record:
                if len(out) >= total:
                    break
                out.append(int(row[s]))
            if int(live[s]) != 1:
                self.codes[r] = int(live[s])
                self.holder[s] = None

    def run(self) -> Tuple[List[List[int]], List[int]]:
        while self.queue or any(r is not None for r in self.holder):
            self._admit()
            record, first = self.driver.step()
            live, left = self.driver.state()
            self.launches += 1
            self._harvest(record, first, live, left)
        return self.tokens, self.codes
