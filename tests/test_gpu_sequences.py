"""The whole device ABI queued back to back (seq_model.py): programs of 12-16 steps over three live
batches run on a fresh ctx with no host synchronisation and no device-to-host copy between the steps,
but for the program's own sync steps; then one fec_sync, and every arena, every word array and every
clone of the words taken on the stream after a call is compared whole with the model. A program
that differs is run again on a new ctx with a sync and a full compare after every step, and the
assertion names the first step that differs there, or says that the program differs only when queued:
a per-call bug in the first case, an ordering or shared-state bug in the second.

Default knobs throughout (the knob forms are covered per call elsewhere).
"""
import pytest

import seq_model as sm
from arena import torch  # noqa: F401

pytestmark = pytest.mark.gpu


def queued(fec, torch, oracle, trace, run):
    """run() queues the trace and compares; a failure is explained by the synced form."""
    try:
        run()
    except AssertionError as e:
        torch.cuda.synchronize()
        where = sm.first_synced_difference(fec, torch, trace, oracle)
        raise AssertionError("%s\n%s\nprogram %d: %s" % (e, where, trace.seed, "; ".join(
            "%d %s %s" % (i, st.kind, st.batch) for i, st in enumerate(trace.steps)))) from None


@pytest.mark.parametrize("seed", range(sm.N_PROGRAMS))
def test_queued_program_matches_model(fec, torch, oracle, seed):
    trace = sm.Trace(oracle, seed)
    c = fec.Codec(0).use_torch_stream()
    try:
        queued(fec, torch, oracle, trace, lambda: sm.run_queued(fec, torch, c, trace, oracle))
    finally:
        torch.cuda.synchronize()
        c.close()


@pytest.mark.parametrize("seed", range(8))
def test_two_contexts_interleaved(fec, torch, oracle, seed):
    """Two ctxs on two streams, two different programs queued alternately step by step from one host
    thread with no waits: each ctx's workspace is its own, and the code caches and the process-wide
    knobs do not interfere."""
    traces = [sm.Trace(oracle, seed), sm.Trace(oracle, sm.N_PROGRAMS - 1 - seed)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [fec.Codec(0), fec.Codec(0)]
    try:
        devs = [sm.Device(fec, torch, c, t, oracle, s) for c, t, s in zip(ctxs, traces, streams)]
        # the uploads ran on torch's streams; the codecs' own streams do not order after them
        torch.cuda.synchronize()
        for c, s in zip(ctxs, streams):
            c.set_stream(s.cuda_stream)

        def run():
            for i in range(max(len(t.steps) for t in traces)):
                for d in devs:
                    if i < len(d.t.steps):
                        d.step(i)
            for d in devs:
                sm.finish(d, "interleaved")
        try:
            run()
        except AssertionError as e:
            torch.cuda.synchronize()
            raise AssertionError("%s\n%s" % (e, "; ".join("program %d: %s" % (
                t.seed, sm.first_synced_difference(fec, torch, t, oracle)) for t in traces))) from None
    finally:
        torch.cuda.synchronize()
        for c in ctxs:
            c.close()


def test_stream_switch_mid_program(fec, torch, oracle):
    """One ctx, the first half of a program over A, D and F on one stream, then fec_ctx_set_stream and the
    second half on another with no host wait: the handoff event orders workspace users of different
    kinds on either side (test_stream_switch_orders_shared_workspace has sorted plans on both)."""
    S = sm.Step
    steps = [
        S("erase", "D", dict(mode="data", seed=1)), S("reconstruct", "D", {}),                  # block-order plans
        S("erase", "F", dict(mode="data", seed=2)), S("reconstruct_wide", "F", {}),             # wide
        S("corrupt", "A", dict(t=2, seed=3)), S("locate_multi", "A", dict(max_bad=8)),          # locate-multi
        # ---- the switch
        S("heal", "A", {}),                                                                     # some, masks from stream 1
        S("erase", "A", dict(mode="data", seed=4)), S("reconstruct", "A", {}),                  # routed
        S("erase", "F", dict(mode="data", seed=5)), S("recover_wide", "F", dict(slots=20)),      # wide
        S("erase", "A", dict(mode="data", seed=6)), S("recover", "A", dict(slots=4)),           # sorted plans
        S("corrupt", "D", dict(t=1, seed=7)), S("locate_multi", "D", dict(max_bad=8)), S("heal", "D", {}),
    ]
    half = 6
    trace = sm.Trace(oracle, 1000, ["A", "D", "F"], steps)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    c = fec.Codec(0)
    try:
        dev = sm.Device(fec, torch, c, trace, oracle, streams[0])
        torch.cuda.synchronize()
        c.set_stream(streams[0].cuda_stream)

        def run():
            for i in range(half):
                dev.step(i)
            c.set_stream(streams[1].cuda_stream)
            dev.stream = streams[1]
            for i in range(half, len(steps)):
                dev.step(i)
            sm.finish(dev, "stream switch")
        queued(fec, torch, oracle, trace, run)
    finally:
        torch.cuda.synchronize()
        c.close()
