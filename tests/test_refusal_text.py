"""The full text of every refusal of the flow family that the CPU tests provoke, held against a recorded table
(tests/golden/refusal_text.json): for the C entries the return code and the whole of soil_last_error(), for the Python
layer the exception's type and the whole of str(e).  The cases are the tables of test_flow_paths_abi, test_downstream_abi,
test_deposit_abi, test_diffuse_abi, test_flats_abi, test_flow_batch_abi and test_fill_batch_abi, which hold the
messages to a prefix only; a case is named by its file, its table and its place or label there.

`python tests/test_refusal_text.py --write` records the table anew.  The table is what the code gave before the
argument checks of soil.py and erosion.py and the host helpers of csrc were made single; it is to be written again
only where a message is meant to change."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "refusal_text.json")


def _c_cases():
    """(key, call): call() returns the entry's return code."""
    import test_deposit_abi, test_diffuse_abi, test_downstream_abi, test_fill_batch_abi, test_flats_abi
    import test_flow_batch_abi, test_flow_paths_abi
    from soillib_amd import _abi
    for what, single, batch in test_flow_paths_abi._calls():
        for name, call in (("flow_paths", single), ("flow_paths_batch", batch)):
            if call is not None:
                yield "flow_paths_abi/%s/%s" % (name, what), call
    for mod in (test_downstream_abi, test_deposit_abi, test_diffuse_abi):
        for name, call in mod._entries().items():
            for what, over in mod._cases(name):
                yield "%s/%s/%s" % (mod.__name__[len("test_"):], name, what), (lambda call=call, over=over: call(over))
    for what, calls in test_flats_abi._calls():
        for name, call in calls.items():
            yield "flats_abi/%s/%s" % (name, what), call
    fill = _abi.lib().soil_fill_depressions_batch
    for what, args in test_fill_batch_abi._refused():
        yield "fill_batch_abi/fill_depressions_batch/%s" % what, (lambda args=args: fill(*args, None))
    for T in test_flow_batch_abi.REFUSED_T:
        for name, rc, msg in test_flow_batch_abi._with_temperature(_abi.lib(), T):
            yield "flow_batch_abi/%s/T %r" % (name, T), (lambda rc=rc, msg=msg: (rc, msg))


def _py_cases():
    """(key, call): call() raises."""
    import test_deposit_abi, test_diffuse_abi, test_downstream_abi, test_fill_batch_abi, test_flats_abi
    import test_flow_batch_abi, test_flow_paths_abi
    for mod in (test_flow_paths_abi, test_downstream_abi, test_deposit_abi, test_diffuse_abi, test_flats_abi,
                test_flow_batch_abi, test_fill_batch_abi):
        short = mod.__name__[len("test_"):]
        for i, case in enumerate(mod._module_refusals()):
            fn, args, kw = case[0], case[1], case[2] if len(case) == 4 else {}
            yield "%s/module/%d %s" % (short, i, fn.__name__), (lambda fn=fn, args=args, kw=kw: fn(*args, **kw))
    for mod in (test_flow_paths_abi, test_downstream_abi, test_deposit_abi, test_diffuse_abi, test_flow_batch_abi):
        short = mod.__name__[len("test_"):]
        for i, (method, scales, args, kw, _) in enumerate(mod._batch_refusals()):
            yield "%s/batch/%d %s" % (short, i, method), (
                lambda mod=mod, method=method, scales=scales, args=args, kw=kw:
                getattr(mod._batch_without_a_device(scales=scales), method)(*args, **kw))
    for i, kw in enumerate(test_flow_batch_abi.FLOW):
        yield "flow_batch_abi/batch/flow %d" % i, (lambda kw=kw: test_flow_batch_abi._batch_without_a_device().flow(**kw))
    for T in test_flow_batch_abi.REFUSED_T:
        yield "flow_batch_abi/batch/flow T %r" % T, (
            lambda T=T: test_flow_batch_abi._batch_without_a_device().flow(kind="random_weighted", T=T))
    for i, (kw, _) in enumerate(test_fill_batch_abi.CONDITIONED):
        yield "fill_batch_abi/batch/%d conditioned" % i, (lambda kw=kw: test_fill_batch_abi._stub().conditioned(**kw))
        if kw.get("kind") == "random_weighted":
            yield "fill_batch_abi/batch/%d flow" % i, (lambda kw=kw: test_fill_batch_abi._stub().flow(**kw))
    yield "fill_batch_abi/batch/filled", lambda: test_fill_batch_abi._stub().filled(edge=7)


def _observe():
    from soillib_amd import _abi
    seen = {}
    for key, call in _c_cases():
        assert key not in seen, key
        got = call()
        rc, msg = got if isinstance(got, tuple) else (got, _abi.last_error())
        seen[key] = {"rc": int(rc), "error": msg}
    for key, call in _py_cases():
        assert key not in seen, key
        try:
            call()
        except Exception as e:                                      # noqa: BLE001 - the type is what is recorded
            seen[key] = {"type": type(e).__name__, "text": str(e)}
        else:
            seen[key] = {"type": None, "text": None}
    return seen


def test_every_refusal_has_the_recorded_text():
    want = json.load(open(GOLDEN))
    got = _observe()
    assert sorted(got) == sorted(want), "the cases of the tables and of the record differ: %r" % (
        sorted(set(got) ^ set(want))[:10],)
    wrong = ["%s: %r, recorded %r" % (k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not wrong, "%d of %d texts moved:\n%s" % (len(wrong), len(want), "\n".join(wrong))
    assert all(v.get("type", "") is not None for v in want.values()), "a recorded case raised nothing"


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_refusal_text.py --write")
    sys.path.insert(0, os.path.dirname(HERE))
    table = _observe()
    with open(GOLDEN, "w") as f:
        json.dump(table, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases written to %s" % (len(table), os.path.relpath(GOLDEN, os.path.dirname(HERE))))
