"""From device tensors to PNG files: the host half of `--save_png`.

A `PictureSet` collects the pictures of one save().  Adding a picture launches its conversion (ops.artefacts: one kernel,
packed 8-bit RGB) on the CURRENT stream and starts the copy of the 3 bytes per pixel into a pinned host buffer on the
same stream; nothing waits.  `write()` waits once for the stream's copies, deflates (helper_functions/png.py) and writes.
Stream order is what protects a pair's static buffers: the next pair of the same shape uploads into them on the same
stream (graph_sets.adopt), after the conversions that read them -- so save() must run with the pair's stream current;
under --pairs_in_flight the drivers see to that (attack_PCFA.PairsInFlight.on_lane).

Inside `with background_writes():` (attack_PCFA.attack_l2) write() only records an event behind the copies and hands the
set to ONE worker thread, which waits for the event, deflates (zlib releases the GIL) and writes while the next pair is
attacked; at most two sets are pending (a third write() blocks), and leaving the block joins the worker and re-raises what
it met.  Measured: profiles/save_png/README.md.
"""
import contextlib
import os
import queue
import threading

import torch

from .. import ops
from . import png

_PINNED = {}   # bytes -> free pinned uint8 buffers (allocating pinned memory costs more than a picture's copy)
_PINNED_LOCK = threading.Lock()   # the worker thread gives buffers back
MAX_PENDING = 2   # picture sets (pairs) the worker may be behind


def _pinned(nbytes):
    with _PINNED_LOCK:
        free = _PINNED.get(nbytes)
        if free:
            return free.pop()
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)


def _release(buf):
    with _PINNED_LOCK:
        free = _PINNED.setdefault(buf.numel(), [])
        if len(free) < 32:
            free.append(buf)


class _Worker:
    """One thread that writes picture sets in the order they were handed over."""

    def __init__(self):
        self.jobs = queue.Queue(maxsize=MAX_PENDING)
        self.error = None
        self.thread = threading.Thread(target=self._run, name="pcfa-png-writer", daemon=True)
        self.thread.start()

    def _run(self):
        while True:
            job = self.jobs.get()
            try:
                if job is None:
                    return
                if self.error is None:      # after a failure the remaining sets are dropped, the error is re-raised at the join
                    job()
            except BaseException as e:  # noqa: BLE001 -- handed to the thread that joins
                self.error = e
            finally:
                self.jobs.task_done()

    def submit(self, job):
        if self.error is not None:
            self.close()
        self.jobs.put(job)      # blocks while MAX_PENDING sets wait

    def close(self):
        self.jobs.put(None)
        self.thread.join()
        if self.error is not None:
            raise self.error


_worker = None


@contextlib.contextmanager
def background_writes():
    """While open, PictureSet.write() of this process returns at once and a worker thread deflates and writes; the exit
    waits for it and re-raises its error.  Not re-entrant."""
    global _worker
    if _worker is not None:
        raise RuntimeError("background_writes() is already open")
    _worker = _Worker()
    try:
        yield
    finally:
        worker, _worker = _worker, None
        worker.close()


def on_device(value, device):
    """A scale as the kernels read it: a float32 device tensor (numbers are uploaded, tensors pass)."""
    if torch.is_tensor(value):
        return value.detach().to(device=device, dtype=torch.float32)
    return torch.full((1,), float(value), device=device, dtype=torch.float32)


def item_paths(filename, items):
    """The reference's batch rule (ownutilities.py:430-441,494-505): item 0 goes to `filename`, item i to
    `filename + "_i.png"`."""
    return [filename if i == 0 else "%s_%d.png" % (filename, i) for i in range(items)]


class PictureSet:
    def __init__(self):
        self._pending = []   # (paths of the B items, pinned buffer, device picture [B,H,W,3]: alive until its copy is done)

    def _fetch(self, rgb, paths):
        if len(paths) != rgb.shape[0]:
            raise ValueError("%d items, %d file names" % (rgb.shape[0], len(paths)))
        buf = _pinned(rgb.numel())
        buf.view(rgb.shape).copy_(rgb, non_blocking=True)
        self._pending.append((list(paths), buf, rgb))

    def add_image(self, paths, x, add=None, normalize_max=None, unit_input=True):
        """(x [+ add]) as an 8-bit picture per item (ops.image_to_rgb8); paths: one file per item, None skips an item."""
        self._fetch(ops.get().image_to_rgb8(x, add=add, normalize_max=normalize_max, unit_input=unit_input), paths)

    def add_flow(self, paths, flow, scale):
        """The colour code of `flow`, item b scaled by scale[b] (ops.flow_to_rgb8)."""
        self._fetch(ops.get().flow_to_rgb8(flow, scale), paths)

    def write(self):
        """Wait for the copies queued so far, then deflate and write every picture; returns the paths written.  Inside
        background_writes() the waiting and writing happen on the worker thread and the paths are returned at once."""
        if not self._pending:
            return []
        event = torch.cuda.Event()
        event.record()
        pending, self._pending = self._pending, []
        if _worker is not None:
            _worker.submit(lambda: self._finish(event, pending))
            return [p for paths, _, _ in pending for p in paths if p is not None]
        return self._finish(event, pending)

    @staticmethod
    def _finish(event, pending):
        event.synchronize()
        written = []
        for paths, buf, rgb in pending:
            host = buf.view(rgb.shape).numpy()
            for b, path in enumerate(paths):
                if path is None:
                    continue
                folder = os.path.dirname(path)
                if folder:
                    os.makedirs(folder, exist_ok=True)
                written.append(png.write_rgb8(path, host[b]))
            _release(buf)
        return written
