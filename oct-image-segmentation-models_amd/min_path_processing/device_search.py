"""Min-path boundary search as a column recurrence: the definition the device kernel implements
(``oct_minpath_device``, include/oct_unet.h; csrc/kernels_minpath.hpp), restated in numpy, the wrapper that runs the
kernel, and the merge that keeps the results identical to the host search.

The grid graph of ``graph_search`` is a DAG by columns: interior vertices have edges only to the next column (right,
``max_grad`` up, ``max_grad`` down) and the "down" edges exist only inside the two appended columns of ones, where they
cost ``2 - (1 + 1) = 0``.  Every edge weight is >= 0 and fp64 addition is monotone, so Dijkstra's final distance of every
vertex is, bit for bit, what the recurrence ``D[j+1][r] = min_r' D[j][r'] + (2.0 - (P[j][r'] + P[j+1][r]))`` produces.
The minimal path cost therefore always equals the host's, and so does the delineation whenever it is unique.  Dijkstra
resolves exact fp64 ties by the push order of its heap, which no column rule reproduces; the recurrence flags every map
whose chosen path passes a tie (``tied``), and ``merge_ties`` sends exactly those maps back to the host search."""
from __future__ import annotations

from typing import Callable, List, Optional, Tuple

import numpy as np

from . import graph_search

MAX_GRAD_RANGE = (1, 16)          # liboct_minpath.so's range


def delineate_dp(maps_u8: np.ndarray, max_grad: int = 1) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(n, M, H, W) uint8 boundary maps -> (rows uint16 (n, M, W), cost float64 (n, M), tied bool (n, M)).

    p = maps / 255 (fp64).  Graph column 0 and W + 1 are ones; D[0][r] = 0.  Per image column j the predecessors of row
    r are tried in the order right (r), below nearest first (r+1..r+max_grad), above nearest first (r-1..r-max_grad);
    the first that attains the minimum is chosen, and the vertex carries a tie bit if more than one attains it and
    j >= 1 (the predecessors in the appended column are all equal and change no delineation).  The path ends at the
    smallest row r' attaining cost = min D[W][r'] + (2.0 - (P[W][r'] + 1.0)) -- the zero-cost last column collapses to
    this -- tied if more than one attains it.  ``tied`` = that end tie OR the tie bits of the vertices on the chosen
    path: a tie bit off the path cannot change it, and another optimal delineation shows where the two paths merge."""
    maps_u8 = np.asarray(maps_u8)
    if maps_u8.dtype != np.uint8 or maps_u8.ndim != 4:
        raise TypeError("maps_u8 must be a (n, M, H, W) uint8 array")
    G = int(max_grad)
    if not MAX_GRAD_RANGE[0] <= G <= MAX_GRAD_RANGE[1]:
        raise ValueError("max_grad must lie in 1..16")
    n, M, H, W = maps_u8.shape
    N = n * M
    P = maps_u8.reshape(N, H, W) / 255
    D, Pc = np.zeros((N, H)), np.ones((N, H))
    choice = np.zeros((N, W, H), np.int8)
    tiebit = np.zeros((N, W, H), bool)
    offsets = [0] + list(range(1, G + 1)) + [-g for g in range(1, G + 1)]
    for j in range(W):
        pn = P[:, :, j]
        best = ch = cnt = None
        for o in offsets:
            lo, hi = max(0, -o), min(H, H - o)              # rows r with 0 <= r + o < H
            if lo >= hi:
                continue
            cand = np.full((N, H), np.inf)
            cand[:, lo:hi] = D[:, lo + o:hi + o] + (2.0 - (Pc[:, lo + o:hi + o] + pn[:, lo:hi]))
            if best is None:
                best, ch, cnt = cand, np.zeros((N, H), np.int8), np.ones((N, H), np.int32)
                continue
            lt, eq = cand < best, cand == best
            best = np.where(lt, cand, best)
            ch = np.where(lt, np.int8(o), ch)
            cnt = np.where(lt, 1, cnt + eq)
        D, Pc = best, pn
        choice[:, j, :] = ch
        if j >= 1:
            tiebit[:, j, :] = cnt > 1
    end = D + (2.0 - (Pc + 1.0))
    cost = end.min(axis=1)
    r = end.argmin(axis=1)                                   # the first, i.e. smallest, row attaining it
    tied = (end == cost[:, None]).sum(axis=1) > 1
    rows = np.zeros((N, W), np.uint16)
    idx = np.arange(N)
    for j in range(W - 1, -1, -1):
        rows[:, j] = r
        tied |= tiebit[idx, j, r]
        r = r + choice[idx, j, r]
    return rows.reshape(n, M, W), cost.reshape(n, M), tied.reshape(n, M)


class _Merged:
    """A batch of ``merge_ties_async``: ``get()`` waits for the host search of its tied maps and returns the results."""

    def __init__(self, rows, truths, where, pending):
        self._rows, self._truths, self._where, self._pending = rows, truths, where, pending

    def get(self) -> List[Tuple[np.ndarray, np.ndarray]]:
        rows, truths = self._rows, self._truths
        if self._pending is not None:
            res = self._pending.get()
            for k, (i, m) in enumerate(zip(*self._where)):
                rows[i, m] = res[k][0][0]
            self._pending = None
        n, M, W = rows.shape
        out = []
        for i in range(n):
            errors = np.zeros((M, W), np.float64)
            if truths is not None:
                for m in range(M):
                    errors[m] = graph_search.calc_errors(rows[i, m], truths[i][m])
            out.append((rows[i], errors))
        return out


class _Ready:
    def __init__(self, res): self._res = res
    def get(self): return self._res


def merge_ties_async(maps_u8: np.ndarray, rows: np.ndarray, tied: np.ndarray, truths: Optional[np.ndarray],
                     segment_async: Callable[[np.ndarray, Optional[np.ndarray]], object], ties: str = "host") -> _Merged:
    """``merge_ties`` with the host search of the tied maps left in flight (``SegmentPool.segment_async``): the caller
    can queue the next device batch before it calls ``get()``."""
    if ties not in ("host", "device"):
        raise ValueError('ties must be "host" or "device"')
    rows = np.array(rows, dtype=np.uint16)
    tied = np.asarray(tied).astype(bool)
    where = pending = None
    if ties == "host" and tied.any():
        where = np.nonzero(tied)
        pending = segment_async(np.ascontiguousarray(maps_u8[where][:, None]), None)       # (k, 1, H, W)
    return _Merged(rows, truths, where, pending)


def merge_ties(maps_u8: np.ndarray, rows: np.ndarray, tied: np.ndarray, truths: Optional[np.ndarray],
               segment: Callable[[np.ndarray, Optional[np.ndarray]], list],
               ties: str = "host") -> List[Tuple[np.ndarray, np.ndarray]]:
    """Results of one batch in the form ``SegmentPool.segment`` returns them -- [(predictions uint16 (M, W), errors
    float64 (M, W)), ...] per image -- from the recurrence's ``rows`` (n, M, W) and ``tied`` (n, M).

    ``ties="host"``: the tied maps, and only those, go through ``segment`` (``SegmentPool.segment``: the host search) as
    one-map images and replace the recurrence's rows: every output equals ``graph_search.segment_maps`` of the same maps.
    ``ties="device"``: ``segment`` is never called.  ``errors`` are ``graph_search.calc_errors`` of the rows (zeros
    without ``truths``, as ``segment_maps`` leaves them)."""
    return merge_ties_async(maps_u8, rows, tied, truths, lambda m, t: _Ready(segment(m, t)), ties).get()


class LazyPool:
    """The host search for the tied maps of ``merge_ties``: a ``SegmentPool`` that is only started when the first tied map
    arrives (clean ridge maps never start it).  ``calls`` counts the batches that needed it."""

    def __init__(self, image_shape_hw, gsgrad: int = 1, workers: Optional[int] = None):
        self._args, self._pool, self.calls = (image_shape_hw, gsgrad, workers), None, 0

    def __call__(self, maps: np.ndarray, truths: Optional[np.ndarray] = None) -> list:
        if self._pool is None:
            from .pool import SegmentPool
            self._pool = SegmentPool(*self._args)
        self.calls += 1
        return self._pool.segment(maps, truths)

    def close(self) -> None:
        if self._pool is not None:
            self._pool.close()
            self._pool = None


class DeviceMinPath:
    """Owns the workspace and the outputs of ``oct_minpath_device`` for up to ``batch`` images of ``M`` boundary maps
    (H, W) and runs it on the current stream.  ``__call__(maps)`` -> (rows (n, M, W) int16 holding uint16 bits,
    cost (n, M) float64, tied (n, M) uint8) on the device; ``to_host`` turns such tensors into numpy uint16 / float64 /
    bool arrays."""

    def __init__(self, batch: int, M: int, H: int, W: int, max_grad: int = 1, device="cuda:0"):
        import torch
        from .. import _hip
        self._hip, self._torch = _hip, torch
        self.B, self.M, self.H, self.W, self.max_grad = int(batch), int(M), int(H), int(W), int(max_grad)
        self.device = torch.device(device)
        nbytes = _hip.lib().oct_minpath_workspace_bytes(self.B, self.M, self.H, self.W, self.max_grad)
        if nbytes == 0:
            raise _hip.OctError(f"oct_minpath_device does not support B={batch}, M={M}, {H}x{W}, max_grad={max_grad}")
        self.workspace = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.rows = torch.empty((self.B, self.M, self.W), dtype=torch.int16, device=self.device)
        self.cost = torch.empty((self.B, self.M), dtype=torch.float64, device=self.device)
        self.tied = torch.empty((self.B, self.M), dtype=torch.uint8, device=self.device)
        self.outs, self.geometry = (self.rows, self.cost, self.tied), (self.B, self.M, self.H, self.W)

    def __call__(self, maps, rows=None, cost=None, tied=None):
        torch, _hip = self._torch, self._hip
        _hip.expect(maps, "maps", device=self.device, dtype=torch.uint8, shape=(None, self.M, self.H, self.W))
        n = maps.shape[0]
        if not 1 <= n <= self.B:
            raise _hip.OctError(f"maps needs a count n in 1..{self.B}, not {n}")
        outs = tuple(_hip.out_view(t, own, n, what) for t, own, what in zip((rows, cost, tied), self.outs, ("rows", "cost", "tied")))
        _hip.call("oct_minpath_device", self.device, maps.data_ptr(), n, self.M, self.H, self.W, self.max_grad,
                  self.workspace.data_ptr(), self.workspace.numel(), *(t.data_ptr() for t in outs), _hip.stream_ptr(self.device))
        return outs

    @staticmethod
    def to_host(rows, cost, tied, first_image: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        # (first_image: what the pipeline's stages take in common; nothing here can fail per image)
        return (rows.cpu().numpy().view(np.uint16).copy(), cost.cpu().numpy().copy(), tied.cpu().numpy().astype(bool))
