"""Host logic of ``serve.DecodeServer(mixed_prefill=True)``: which waiting prefills share a pass, which engine entry the pass goes through and how its
logits are handed back - on stand-in pools and a recording stand-in engine (no device: the HIP stream / event objects the server creates are replaced by
inert ones)."""
import contextlib
from types import SimpleNamespace

import pytest
import torch

from revisionllm_amd import serve

V = 5


class _Event:
    def record(self, stream=None):
        pass

    def query(self):
        return True

    def synchronize(self):
        pass


class _Stream:
    def __init__(self, device=None):
        pass

    def wait_event(self, ev):
        pass


class _H(torch.Tensor):
    """Host rows standing in for a ticket's device tensor."""

    def record_stream(self, stream):
        pass


class _Engine:
    """Records the prefill entries the server calls; logits row i holds the value i (so a ticket's slice shows which rows it was given)."""

    def __init__(self):
        self.device, self.slot, self.calls = torch.device("cpu"), 0, []

    @staticmethod
    def _logits(n):
        return torch.arange(n, dtype=torch.float32)[:, None].expand(n, V).contiguous()

    def llm_prefill_pool(self, h, B, P0, kv, kv_rows, kv_row0, Smax, logits=None):
        self.calls.append(("pool", B, P0, int(h.shape[0]), kv_rows, kv_row0, Smax))
        return self._logits(B)

    def llm_prefill_pool_groups(self, h, G, B, P0, kv, kv_rows, row0s, Smax, logits=None, last_rows=None):
        self.calls.append(("groups", G, B, P0, int(h.shape[0]), kv_rows, list(row0s), Smax, None if last_rows is None else last_rows.tolist()))
        return self._logits(G * B)

    def llm_prefill_pool_mixed(self, h, groups, kv, R, Smax, last_rows=None, logits=None):
        self.calls.append(("mixed", [tuple(g) for g in groups], int(h.shape[0]), R, Smax, None if last_rows is None else last_rows.tolist()))
        return self._logits(sum(g[0] for g in groups))


class _Pool:
    def __init__(self, model, rows, smax, gmax, max_ahead, slot, gang):
        self.R, self.Smax, self.kv = rows, smax, object()

    def pump(self):
        return False


@pytest.fixture
def inert_streams(monkeypatch):
    monkeypatch.setattr(torch.cuda, "Event", _Event)
    monkeypatch.setattr(torch.cuda, "Stream", _Stream)
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())


def _server(mixed, pools=2, **kw):
    eng = _Engine()
    if mixed is None:
        sv = serve.DecodeServer(SimpleNamespace(engine=eng), rows=64, smax=256, gmax=16, pools=pools, gang=True, prefill_batch=4, pool_factory=_Pool, **kw)
    else:
        sv = serve.DecodeServer(SimpleNamespace(engine=eng), rows=64, smax=256, gmax=16, pools=pools, gang=True, prefill_batch=4, pool_factory=_Pool,
                                mixed_prefill=mixed, **kw)
    return sv, eng


def _submit(sv, pool, r0, B, P0, S, lens=None):
    job = serve.Job(r0, B)
    job.pool = pool
    return sv.submit_prefill(job, torch.zeros(P0 + B * S, 2).as_subclass(_H), B, P0, lens)


GEOMS = [(7, 32, 139), (7, 32, 131), (7, 32, 150), (5, 32, 139)]      # rows 1005, 949, 1082, 727: 15 row tiles of 256 together
ROW0 = [0, 7, 14, 21]


def _drain(sv):
    n = 0
    while sv.pf_queue:
        assert sv._pump_prefill(force=True)
        n += 1
        assert n < 32
    return n


def test_best_prefill_count_is_the_batch_rule_on_cumulative_rows():
    for rows in (72, 327, 1005):
        for avail in range(1, 9):
            assert serve.best_prefill_count([rows] * avail) == serve.best_prefill_batch(avail, rows)
    rows = [P0 + B * S for B, P0, S in GEOMS]
    assert serve.best_prefill_count(rows) == 4                    # 15 row tiles fill 30 of an XCD's 32 CUs: 4.0 tiles per prefill, ties go to the larger batch
    assert serve.best_prefill_count([1005, 1005, 1100]) == 2      # 8 tiles (every CU busy) beat 13 tiles on 26 of 32 CUs
    assert serve.best_prefill_count([72]) == 1 and serve.best_prefill_count([]) == 1


def test_four_tickets_of_different_geometry_share_one_pass(inert_streams):
    sv, eng = _server(True)
    pool = sv.pools[0]
    tickets = [_submit(sv, pool, r0, *g) for r0, g in zip(ROW0, GEOMS)]
    assert sv.pump()                                                # a full batch (prefill_batch = 4) goes at once
    assert not sv.pf_queue and len(eng.calls) == 1
    kind, groups, rows, R, Smax, last = eng.calls[0]
    assert kind == "mixed" and groups == [(B, P0, S, r0) for (B, P0, S), r0 in zip(GEOMS, ROW0)]
    assert rows == sum(P0 + B * S for B, P0, S in GEOMS) and (R, Smax) == (pool.R, pool.Smax) and last is None
    assert sv.pf_batches == 1 and sv.pf_tickets == 4 and sv.pf_hist == {4: 4}
    # the logits slices follow cumulative B: 7, 7, 7, 5
    row = 0
    for t, (B, _, _) in zip(tickets, GEOMS):
        assert t.ready is not None and t.h is None and t.first.shape == (B, V)
        assert t.first[:, 0].tolist() == list(range(row, row + B))
        row += B


def test_without_mixing_the_calls_are_those_of_the_uniform_server(inert_streams):
    """``mixed_prefill=False`` (and the default): a ticket of another geometry closes the group - four passes of one ticket, each through
    ``llm_prefill_pool`` with its own rows, in submission order; identical geometry goes through ``llm_prefill_pool_groups``, mixing on or off."""
    for mixed in (False, None):
        sv, eng = _server(mixed)
        assert sv.mixed_prefill is False
        pool = sv.pools[0]
        tickets = [_submit(sv, pool, r0, *g) for r0, g in zip(ROW0, GEOMS)]
        assert _drain(sv) == 4
        assert eng.calls == [("pool", B, P0, P0 + B * S, pool.R, r0, pool.Smax) for (B, P0, S), r0 in zip(GEOMS, ROW0)]
        assert sv.pf_hist == {1: 4} and sv.pf_batches == 4 and sv.pf_tickets == 4
        assert all(t.first[:, 0].tolist() == list(range(t.B)) for t in tickets)
    want = None
    for mixed in (False, True):
        sv, eng = _server(mixed)
        pool = sv.pools[0]
        for r0 in ROW0:
            _submit(sv, pool, r0, 7, 32, 139)
        assert sv.pump() and not sv.pf_queue
        assert eng.calls == [("groups", 4, 7, 32, 4 * 1005, pool.R, ROW0, pool.Smax, None)]
        want = want or eng.calls
        assert eng.calls == want and sv.pf_hist == {4: 4}


def test_tickets_of_different_pools_or_outside_the_limits_never_mix(inert_streams):
    sv, eng = _server(True)
    a, b = sv.pools
    _submit(sv, a, 0, 7, 32, 139)
    _submit(sv, a, 7, 5, 32, 120)
    _submit(sv, b, 0, 7, 32, 131)
    _submit(sv, b, 7, 3, 40, 99)
    assert _drain(sv) == 2
    assert [c[0] for c in eng.calls] == ["mixed", "mixed"]
    assert eng.calls[0][1] == [(7, 32, 139, 0), (5, 32, 120, 7)] and eng.calls[1][1] == [(7, 32, 131, 0), (3, 40, 99, 7)]
    assert sv.pf_hist == {2: 4}
    # S <= 16, 0 < P0 <= 16 and P0 + S > Smax lie outside the entry's limits, and a sequence shorter than 32 positions does not share a pass with longer
    # ones (its last block takes another form): such a ticket closes the group in front of it and goes alone
    for bad in [(1, 0, 10), (2, 8, 40), (1, 0, 300), (1, 0, 20)]:
        sv, eng = _server(True)
        pool = sv.pools[0]
        _submit(sv, pool, 0, 7, 32, 139)
        _submit(sv, pool, 7, 7, 32, 120)
        _submit(sv, pool, 14, *bad)
        _submit(sv, pool, 20, 7, 32, 100)
        assert _drain(sv) == 3
        assert [c[0] for c in eng.calls] == ["mixed", "pool", "pool"], bad
        assert eng.calls[0][1] == [(7, 32, 139, 0), (7, 32, 120, 7)]
        assert eng.calls[1][1:4] == (bad[0], bad[1], bad[1] + bad[0] * bad[2])
    # a lead ticket outside the limits still batches with tickets of ITS geometry, through the uniform entry
    sv, eng = _server(True)
    pool = sv.pools[0]
    _submit(sv, pool, 0, 2, 8, 40)
    _submit(sv, pool, 2, 2, 8, 40)
    _submit(sv, pool, 4, 7, 32, 100)
    assert _drain(sv) == 2
    assert eng.calls[0] == ("groups", 2, 2, 8, 2 * 88, pool.R, [0, 2], pool.Smax, None) and eng.calls[1][0] == "pool"


def test_ragged_tickets_contribute_their_own_last_rows(inert_streams):
    sv, eng = _server(True)
    pool = sv.pools[0]
    _submit(sv, pool, 0, 2, 32, 40)                          # rows 0 .. 111
    _submit(sv, pool, 2, 3, 20, 30, lens=(50, 45, 38))       # rows 112 .. 221: prefix 20, sequences of 30 rows, valid lengths (prefix included) 50 / 45 / 38
    assert _drain(sv) == 1
    kind, groups, rows, _, _, last = eng.calls[0]
    assert kind == "mixed" and groups == [(2, 32, 40, 0), (3, 20, 30, 2)] and rows == 112 + 110
    assert last == [32 + 39, 32 + 79, 112 + 20 + 29, 112 + 20 + 30 + 24, 112 + 20 + 60 + 17]


def test_the_server_does_not_mix_when_the_engine_cannot(inert_streams):
    """The mixed entry refuses the parity precision and the FP8 prefill path (``Engine.mixed_prefill_supported``): the server then keeps to one geometry."""
    sv, eng = _server(True)
    eng.mixed_prefill_supported = lambda: False
    pool = sv.pools[0]
    for r0, g in zip(ROW0, GEOMS):
        _submit(sv, pool, r0, *g)
    assert _drain(sv) == 4 and [c[0] for c in eng.calls] == ["pool"] * 4
