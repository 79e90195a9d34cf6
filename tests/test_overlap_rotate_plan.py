"""CPU: the index arithmetic of the rotating overlapped pipeline
(gx_api_batch.cpp overlap_rotate_plan, exported as gx_overlap_rotate_plan; the
driver pipeline_rotate calls the same function).  Fill i = 2 pass + group
takes FillJob i % 3, a fill slot, a walk slot and a stream; its stream waits
on the device for one earlier walk; and the host has collected some fills and
labelled some walks before it enqueues fill i.  Replaying the driver's enqueue
order for up to 9 passes: no job, slot or pinned block is reused before its
last reader was collected, every wait names an earlier enqueue, and at most
three groups are alive.  No GPU call."""
import pytest


def _driver_order(N):
    """The driver's host loop: tick t collects fill t - 3, enqueues fill t (and
    its walk), then labels pass (t - 3) / 2 once its second group was collected."""
    ev = []
    for t in range(N + 3):
        if t >= 3:
            ev.append(("collect", t - 3))
        if t < N:
            ev.append(("enqueue", t))
        if t >= 3 and (t - 3) % 2 == 1:
            ev.append(("label", (t - 3) // 2))
    return ev


@pytest.mark.parametrize("K", range(2, 10))
def test_rotation_replay(gx, K):
    N = 2 * K
    plan = [gx.overlap_rotate_plan(i) for i in range(N)]
    for i, p in enumerate(plan):
        assert p["job"] == i % 3 and p["stream"] == i % 2 and 0 <= p["fslot"] < 4 and 0 <= p["wslot"] < 6
        # a stream's fills keep to their own pair of fill slots (run_fill looks descriptors up in slot and slot ^ 1)
        assert p["fslot"] // 2 == p["stream"]
    collected, labelled, enq = -1, -1, -1   # the last fill collected, walk labelled, fill enqueued
    job_user, fslot_user, wslot_user = {}, {}, {}
    peak = 0
    for what, x in _driver_order(N):
        if what == "collect":
            assert x == collected + 1 and x <= enq   # in order, and only what was enqueued
            collected = x
        elif what == "label":
            assert 2 * x + 1 <= collected   # both groups' fills collected (the results the labelling reads)
            assert 2 * x + 1 == labelled + 2
            labelled = 2 * x + 1
        else:
            i, p = x, plan[x]
            assert i == enq + 1
            # what the plan says the host has done by now is what the driver did
            assert p["collected"] == collected and p["labelled"] == labelled, (i, p, collected, labelled)
            # every wait names an earlier enqueue
            assert p["wait_walk"] < i
            if p["job"] in job_user:   # the job's last fill: collected on the host, its walk waited for on the device
                j = job_user[p["job"]]
                assert j <= collected and j <= p["wait_walk"], (i, j)
            else:
                assert p["wait_walk"] == -1
            if p["fslot"] in fslot_user:   # pinned results and events of the slot's last fill: collected
                assert fslot_user[p["fslot"]] <= collected, i
            if p["wslot"] in wslot_user:   # pinned records of the slot's last walk: labelled
                assert wslot_user[p["wslot"]] <= labelled, i
            job_user[p["job"]] = fslot_user[p["fslot"]] = wslot_user[p["wslot"]] = i
            enq = i
            # groups alive: enqueued fills whose buffers the host has not released
            peak = max(peak, enq - collected)
    assert collected == N - 1 and labelled == N - 1 and enq == N - 1
    assert peak == 3


def test_plan_rejects_bad_arguments(gx):
    with pytest.raises(gx.GxError):
        gx.overlap_rotate_plan(-1)
