"""CPU suite: the size plan's host-side bookkeeping (cnrma_amd.plan), no device involved."""


def test_plan_copy_is_a_fresh_plan_with_the_same_records():
    """Plan.copy(): equal sizes, flags, marks, margin and slack in lists of its own; a recording plan (not static) without the
    trace state of the original (arena, constants, pinned buffers)"""
    from cnrma_amd.plan import Plan
    p = Plan(1.5, 32)
    for n in (7, 300, 12):
        p.record(n)
    p.record_flag(True)
    p.mark("net")
    p.record(5)
    p.record_flag(False)
    p.begin_static()                           # the original has been traced: none of that travels
    p._arena_need, p._arena_dev = 4096, "cpu"
    p._consts.append(object())
    p.keep(object())
    q = p.copy()
    assert (q.sizes, q.flags, q.marks) == (p.sizes, p.flags, p.marks) == ([7, 300, 12, 5], [True, False], {"net": (3, 1)})
    assert (q.margin, q.slack) == (p.margin, p.slack) == (1.5, 32)
    assert q.sizes is not p.sizes and q.flags is not p.flags and q.marks is not p.marks
    q.sizes[0], q.flags[0] = 99, None
    q.marks["x"] = (0, 0)
    assert p.sizes[0] == 7 and p.flags[0] is True and "x" not in p.marks
    assert q.static is False and getattr(q, "_arena", None) is None and getattr(q, "_arena_need", 0) == 0
    assert q._consts == [] and q._kept == {} and q.workspaces == {}
    q.record(1)                                # still records
    assert len(q.sizes) == len(p.sizes) + 1
