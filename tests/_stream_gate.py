"""A gate for the stream tests (tests/test_streams.py): a bounded piece of device work that keeps one side stream busy
while launches on every other stream run and finish.  TEST SEAM ONLY.

The gate is `torch.cuda._sleep(cycles)`: one thread that reads the clock until ``cycles`` have passed.  It ends by
itself whatever the host does, occupies one wave of one compute unit, and writes no memory.  Nothing here waits for the
host, so nothing here can hang.

A gated call (`gated`):

    inputs hold valid values A, device synchronised
    on the side stream S:      the gate, copies of valid values B into the same input buffers, the call under test, an event
    on the default stream:     the control -- the same call on the same input buffers, into outputs of its own

A side stream of PyTorch does not wait for the legacy default stream and is not waited for by it.  A launch that the call
under test sent to S runs after the gate and reads B; a launch it sent anywhere else, like the control, runs under the gate
and reads A.  The control is the proof, on this machine in this run, that the gate held: if the control read B the test
fails and says so (`check_control`).  The event tells whether the call drained S or the device before it returned."""
from __future__ import annotations

import torch

DEV = "cuda:0"
CAP_SECONDS = 0.5      # a gate is never longer: every test stays within a few seconds
FLOOR_SECONDS = 0.1    # nor shorter: the host side of a gated sequence (Python, ctypes, launches) is milliseconds
MARGIN = 20            # the gate lasts at least this many times the slowest call under test
PROBE_CYCLES = 20_000_000


def seconds_on(stream, work) -> float:
    """Device seconds of ``work()`` enqueued on ``stream``, between two events on it.  Synchronises."""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        t0.record()
        work()
        t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e-3


class Gate:
    """The side stream S and a gate sized for it, once per session: the clock's rate is measured with two events on S after a
    warm-up, the gate is set to 2 * MARGIN times ``slowest_call`` (seconds of the slowest call under test, measured alone on
    the default stream by the caller) within [FLOOR_SECONDS, 0.9 * CAP_SECONDS], and then measured itself."""

    def __init__(self, slowest_call: float):
        self.stream = torch.cuda.Stream(device=DEV)
        self.slowest_call = float(slowest_call)
        seconds_on(self.stream, lambda: torch.cuda._sleep(PROBE_CYCLES // 10))   # warm-up: the kernel's code is loaded
        rate = PROBE_CYCLES / seconds_on(self.stream, lambda: torch.cuda._sleep(PROBE_CYCLES))
        target = min(max(2 * MARGIN * self.slowest_call, FLOOR_SECONDS), 0.9 * CAP_SECONDS)
        self.cycles = int(rate * target)
        self.seconds = seconds_on(self.stream, self.close)
        assert self.seconds <= CAP_SECONDS, f"the gate of {self.cycles} cycles took {self.seconds:.3f} s: over the cap"
        assert self.seconds >= MARGIN * self.slowest_call, \
            f"the gate ({self.seconds * 1e3:.1f} ms) is shorter than {MARGIN} x the slowest call ({self.slowest_call * 1e3:.3f} ms)"
        # a small block of S's own in the caching allocator: tensors made inside `with torch.cuda.stream(S)` come from it
        with torch.cuda.stream(self.stream):
            torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()

    def close(self) -> None:
        """Enqueues the gate on torch's current stream."""
        torch.cuda._sleep(self.cycles)

    def __repr__(self):
        return f"gate of {self.seconds * 1e3:.1f} ms on a side stream (slowest call {self.slowest_call * 1e3:.3f} ms)"


def gated(gate: Gate, write_b, call, control) -> None:
    """The gated call of the module docstring.  ``write_b()`` enqueues the copies of B into the input buffers (device to
    device: nothing that waits), ``call()`` is the call under test, ``control()`` the control; all three use torch's current
    stream.  Returns after one `torch.cuda.synchronize()`.  Asserts that the event recorded behind the call had not happened
    when the call returned (the call neither drained S nor synchronised the device), and has happened after the
    synchronise."""
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(gate.stream):
        gate.close()
        write_b()
        call()
        done.record()
    happened = done.query()
    control()
    torch.cuda.synchronize()
    assert not happened, f"the call under test returned only after the {gate} had ended: it waited for its stream or the device"
    assert done.query()


def check_control(saw_a: bool, saw_b: bool, gate: Gate, what: str) -> None:
    """The control's outputs are A's definition and not B's."""
    assert not saw_b, (f"{what}: the control on the default stream read B -- the {gate} did not hold B back until the control "
                       f"had run, so this run proves nothing about the call under test")
    assert saw_a, f"{what}: the control's outputs are neither A's definition nor B's"
