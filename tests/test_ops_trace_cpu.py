"""The contract of the wrappers in ``reni_amd.ops`` below ``class Plan``, held on the CPU: which entry point each one calls,
with which arguments in which roles, what it asks the ``*_bytes`` functions, what it returns, and which exception a bad
argument raises before and behind the device check.  tests/ops_trace_cases.py has the cases and the recorder;
tests/golden/ops_trace.txt was recorded from the commit before the wrappers' shared checks were merged
(profiles/ops_refactor.md), and this test only compares.  Nothing is launched, no device is needed."""
import os

from tests import ops_trace_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ops_trace.txt")


def test_every_wrapper_calls_the_library_as_recorded(monkeypatch):
    from reni_amd import _lib, ops

    def install(rec):
        monkeypatch.setattr(ops, "_require_cuda", rec.require_cuda)
        monkeypatch.setattr(ops, "_call", rec.call)
        monkeypatch.setattr(_lib, "load", rec.load)

    got, workspaces = C.trace(install, monkeypatch.undo)
    with open(GOLDEN) as f:
        want = f.read().splitlines()
    diff = [f"line {i + 1}:\n  want {w}\n  got  {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff, "\n".join(diff[:20])
    assert len(got) == len(want)
    # every workspace pointer that reaches an entry point is 256-byte aligned by the wrapper itself, not by the allocator
    # (the CPU allocator aligns to 64, so reliance on it shows here)
    assert workspaces
    off = sorted({name for name, p in workspaces if p % 256})
    assert not off, f"workspace pointers off 256-byte alignment: {off}"
