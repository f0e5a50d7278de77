"""`chain_step.HandOver`, the meeting of the two host threads that issue a stage-2 step's chains, with two plain threads and no GPU:
the event it passes along is an opaque object."""
import threading
import time

import pytest

from temporalalignnet_amd._lib import TanHipError
from temporalalignnet_amd.chain_step import HandOver


def _in_thread(fn):
    """run `fn` on a second thread -> (thread, box); box holds ("ok", result) or ("err", exception) once it is through"""
    box, started = [], threading.Event()

    def run():
        started.set()
        try:
            box.append(("ok", fn()))
        except BaseException as e:      # noqa: B902 -- the test looks at it
            box.append(("err", e))
    th = threading.Thread(target=run, daemon=True)
    th.start()
    assert started.wait(5.0)
    return th, box


def test_published_objects_reach_the_waiter_before_and_after_the_wait_began():
    h = HandOver(("early", "late"), timeout=30.0)
    first, second = object(), object()
    h.publish("early", first)                        # published before anybody waits
    assert h.wait("early") is first
    th, box = _in_thread(lambda: h.wait("late"))     # the waiter is (about to be) blocked when the other thread publishes
    h.publish("late", second)
    th.join(5.0)
    assert not th.is_alive() and box == [("ok", second)]
    assert h.wait("late") is second and h.wait("early") is first         # (a name can be waited for again)


def test_a_failed_chain_wakes_the_waiter_with_the_consequence_error():
    h = HandOver(("tgt", "g"), timeout=30.0)
    t0 = time.perf_counter()
    th, box = _in_thread(lambda: h.wait("g"))        # "g" is never published
    h.fail("joint")
    th.join(5.0)
    assert not th.is_alive() and time.perf_counter() - t0 < 5.0         # not after the 30 s
    kind, err = box[0]
    assert kind == "err" and isinstance(err, TanHipError) and err.tan_consequence is True
    assert "did not reach 'g'" in str(err) and "(joint chain failed)" in str(err)
    # a name that WAS published is refused as well once a chain has failed: the step is lost either way
    h.publish("tgt", object())
    with pytest.raises(TanHipError, match="joint chain failed") as ei:
        h.wait("tgt")
    assert ei.value.tan_consequence is True


def test_an_unpublished_name_times_out_with_did_not_reach():
    h = HandOver(("tgt",), timeout=0.2)
    t0 = time.perf_counter()
    with pytest.raises(TanHipError, match="the other chain did not reach 'tgt'") as ei:
        h.wait("tgt")
    assert 0.19 <= time.perf_counter() - t0 < 5.0
    assert ei.value.tan_consequence is True and "chain failed" not in str(ei.value)
