"""Helpers for tests that call the device-resident API on a caller's stream behind pending work (tests/test_gpu_ple_exact.py,
tests/test_gpu_stream_order.py).

The method: a fresh torch stream (torch streams are non-blocking: nothing orders them against the NULL stream) first gets a long
sleep, then the copies that write the inputs into tensors that hold a poison pattern until then, then the library calls, then the
torch ops that read the results -- and only after that does anything synchronise.  A step of the library that strays onto another
stream, or onto the host, runs while the sleep still holds the stream back: it sees the poison instead of its inputs, or its
result is overwritten or read before the work it depends on has run, and the comparison on the host fails."""
import numpy as np

SLEEP_CYCLES = 200_000_000  # torch.cuda._sleep: ~0.1 s of the stream's time
POISON = 0x5A5A5A5A5A5A5A5A  # what an input tensor holds until the stream's copy writes it


def padded(words):
    """the words of a matrix with an even row stride (gf2_dmat: ld even; a zero column is appended to an odd width)"""
    words = np.ascontiguousarray(words)
    if words.shape[1] & 1:
        words = np.hstack([words, np.zeros((words.shape[0], 1), dtype=np.uint64)])
    return np.ascontiguousarray(words)


class Lane:
    """One caller stream.  Lane(arrays) stages the arrays on the device and creates the poisoned tensors `live`; after a device
    synchronisation (lanes() does it) open() queues the sleep and the copies into `live` on the stream; read() queues the reading
    torch ops there and returns host arrays.  Between open() and read() the test makes its library calls with `handle`."""

    def __init__(self, arrays, sleep=1):
        import torch
        self.stream = torch.cuda.Stream()
        self.handle = self.stream.cuda_stream
        self.staged = [torch.from_numpy(np.array(x, dtype=np.uint64, order="C").view(np.int64)).cuda() for x in arrays]
        self.live = [torch.full_like(x, POISON) for x in self.staged]
        self.sleep = int(sleep)  # in units of SLEEP_CYCLES; 0: no sleep
        self.awake = None

    def open(self, only=None):
        """the sleep, an event `awake` right behind it, then the copies into live[i] (i in `only`, default: all)"""
        import torch
        with torch.cuda.stream(self.stream):
            for _ in range(self.sleep):
                torch.cuda._sleep(SLEEP_CYCLES)
            self.awake = torch.cuda.Event()
            self.awake.record(self.stream)
            for i in (range(len(self.live)) if only is None else only):
                self.live[i].copy_(self.staged[i], non_blocking=True)
        return self

    def poison(self):
        """the inputs unwritten again (on the current stream: synchronise before the next open())"""
        for d in self.live:
            d.fill_(POISON)

    def snapshot(self, tensors):
        """device copies of `tensors` as they are at this point of the stream (for intermediates that later calls overwrite)"""
        import torch
        with torch.cuda.stream(self.stream):
            return [t.clone() for t in tensors]

    def read(self, tensors=None):
        import torch
        with torch.cuda.stream(self.stream):
            outs = [t.clone() for t in (self.live if tensors is None else tensors)]
            host = [o.cpu() for o in outs]
        return [h.numpy().view(np.uint64) for h in host]

    def pending(self):
        return not self.stream.query()


def lanes(*array_lists, sleep=1):
    """one Lane per list of arrays, staged and poisoned, the device quiet: ready for open()"""
    import torch
    out = [Lane(arrays, sleep) for arrays in array_lists]
    torch.cuda.synchronize()
    return out


def run_pending(array_lists, issue, check):
    """For ASYNCHRONOUS calls: one lane per list of arrays, all opened; issue(lanes) makes the library calls, check(result of
    issue, [lane.read() for every lane]) compares.  The run only proves something if the streams were still held back when the
    last call had been issued; should the host have been slower than the sleep, the whole run is repeated behind a longer one
    (every run is checked)."""
    for sleep in (1, 4, 16):
        ls = lanes(*array_lists, sleep=sleep)
        for ln in ls:
            ln.open()
        res = issue(ls)
        busy = all(ln.pending() for ln in ls)
        check(res, [ln.read() for ln in ls])
        if busy:
            return
        print("the streams had drained before all calls were issued behind %d sleep(s): repeating behind a longer one" % sleep)
    raise AssertionError("the streams never outlasted the host: the calls were not made behind pending work")


def on_stream(dev, fn_inputs, call):
    """Queue a long sleep on a fresh stream, write the inputs there, make the call there and read the results with a torch op on
    that stream before anything synchronises the device: a step on another stream sees unwritten inputs or unfinished work."""
    (lane,) = lanes(fn_inputs)
    lane.open()
    res = call(lane.live, lane.handle)
    return res, lane.read()
