"""Connected components of the class map: island removal and lesion counts on the device
(``oct_components`` / ``oct_component_filter``, include/oct_unet.h; ``common.utils.components_reference`` and
``component_filter_reference`` restate them bit for bit).  Here: the rule a user states, the wrapper the inference pipeline
runs as a stage and the host formulas of what the result files state about it.  The reference has no counterpart."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple, Union

import numpy as np

from ..common.utils import (COMPONENTS_FILL_COLUMN, COMPONENTS_FILL_CONSTANT, COMPONENTS_MAX_BATCH, COMPONENTS_MAX_CLASSES,
                            component_filter_reference, components_reference)


class ComponentRule:
    """What to remove from a class map and what to put there.

    ``connectivity``  4 or 8.
    ``min_pixels``    one count for every class or a list with a count per class: components with fewer pixels are removed
                      (0 or 1: none).
    ``keep_largest``  the classes of which only the largest component of each image stays: a list of class indices, ``"all"``
                      or nothing.  Among equally large components the one whose first pixel (row-major) comes first stays.
    ``fill``          ``"column"``: a removed pixel takes the label of the nearest kept pixel above it in its column, else of
                      the nearest below it, else 0 -- the rule that suits B-scans; or an int 0..255, the label every removed
                      pixel gets.
    The rule validates what does not depend on the class count when it is built and the rest in ``check(num_classes)``."""

    def __init__(self, connectivity: int = 8, min_pixels: Union[int, Sequence[int]] = 0,
                 keep_largest: Union[str, Sequence[int]] = (), fill: Union[str, int] = "column"):
        if isinstance(connectivity, bool) or connectivity not in (4, 8):
            raise ValueError(f"ComponentRule: connectivity must be 4 or 8, not {connectivity!r}")
        self.connectivity = int(connectivity)
        if isinstance(min_pixels, (int, np.integer)) and not isinstance(min_pixels, bool):
            self.min_pixels: Union[int, Tuple[int, ...]] = int(min_pixels)
            counts = [self.min_pixels]
        elif isinstance(min_pixels, (list, tuple, np.ndarray)) and len(min_pixels) and all(
                isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in min_pixels):
            self.min_pixels = tuple(int(v) for v in min_pixels)
            counts = list(self.min_pixels)
        else:
            raise ValueError(f"ComponentRule: min_pixels must be an int or a non-empty list of ints, not {min_pixels!r}")
        if any(not 0 <= v < 1 << 32 for v in counts):
            raise ValueError(f"ComponentRule: min_pixels must lie in 0..2^32-1, not {min_pixels!r}")
        if isinstance(keep_largest, str):
            if keep_largest != "all":
                raise ValueError(f"ComponentRule: keep_largest must be 'all' or a list of classes, not {keep_largest!r}")
            self.keep_largest: Union[str, Tuple[int, ...]] = "all"
        elif isinstance(keep_largest, (list, tuple, np.ndarray)) and all(
                isinstance(v, (int, np.integer)) and not isinstance(v, bool) for v in keep_largest):
            self.keep_largest = tuple(sorted(int(v) for v in keep_largest))
            if len(set(self.keep_largest)) != len(self.keep_largest) or any(
                    not 0 <= v < COMPONENTS_MAX_CLASSES for v in self.keep_largest):
                raise ValueError(f"ComponentRule: keep_largest needs distinct classes in 0..{COMPONENTS_MAX_CLASSES - 1}, "
                                 f"not {keep_largest!r}")
        else:
            raise ValueError(f"ComponentRule: keep_largest must be 'all' or a list of classes, not {keep_largest!r}")
        if isinstance(fill, str):
            if fill != "column":
                raise ValueError(f"ComponentRule: fill must be 'column' or a label 0..255, not {fill!r}")
            self.fill: Union[str, int] = "column"
        elif isinstance(fill, (int, np.integer)) and not isinstance(fill, bool) and 0 <= int(fill) <= 255:
            self.fill = int(fill)
        else:
            raise ValueError(f"ComponentRule: fill must be 'column' or a label 0..255, not {fill!r}")

    @classmethod
    def coerce(cls, rule, what: str = "components") -> Optional["ComponentRule"]:
        """``None`` | ``ComponentRule`` | a dict of its keywords -> ``None`` | ``ComponentRule``."""
        if rule is None or isinstance(rule, cls):
            return rule
        if isinstance(rule, dict):
            try:
                return cls(**rule)
            except TypeError as e:
                raise ValueError(f"{what}: {e}") from None
        raise ValueError(f"{what} must be None, a ComponentRule or a dict of its keywords, not {rule!r}")

    def as_dict(self) -> dict:
        return {"connectivity": self.connectivity,
                "min_pixels": self.min_pixels if isinstance(self.min_pixels, int) else list(self.min_pixels),
                "keep_largest": self.keep_largest if isinstance(self.keep_largest, str) else list(self.keep_largest),
                "fill": self.fill}

    def __eq__(self, other):
        return isinstance(other, ComponentRule) and self.as_dict() == other.as_dict()

    def __hash__(self):
        return hash(repr(self))

    def __repr__(self):
        return "ComponentRule(" + ", ".join(f"{k}={v!r}" for k, v in self.as_dict().items()) + ")"

    def check(self, num_classes: int, what: str = "components") -> None:
        """Raise ``ValueError`` unless the rule fits ``num_classes`` classes."""
        C = int(num_classes)
        if not 1 <= C <= COMPONENTS_MAX_CLASSES:
            raise ValueError(f"{what}: needs 1..{COMPONENTS_MAX_CLASSES} classes, not {num_classes}")
        if not isinstance(self.min_pixels, int) and len(self.min_pixels) != C:
            raise ValueError(f"{what}: min_pixels has {len(self.min_pixels)} entries for {C} classes")
        if not isinstance(self.keep_largest, str) and any(v >= C for v in self.keep_largest):
            raise ValueError(f"{what}: keep_largest names a class outside 0..{C - 1}: {list(self.keep_largest)}")

    def pack(self, num_classes: int):
        """The rule as the ``oct_component_rule`` of ``num_classes`` classes (``_hip.ComponentRuleC``)."""
        from .. import _hip
        self.check(num_classes)
        C = int(num_classes)
        r = _hip.ComponentRuleC()
        for c in range(C):
            r.min_pixels[c] = self.min_pixels if isinstance(self.min_pixels, int) else self.min_pixels[c]
        classes = range(C) if self.keep_largest == "all" else self.keep_largest
        r.keep_largest = sum(1 << c for c in classes)
        r.fill_mode = COMPONENTS_FILL_COLUMN if self.fill == "column" else COMPONENTS_FILL_CONSTANT
        r.fill_label = 0 if self.fill == "column" else self.fill
        return r


def check_components(num_classes: int, H: int, W: int, what: str = "components") -> None:
    """Raise ``ValueError`` for a class count or image size the component calls refuse."""
    if not 1 <= int(num_classes) <= COMPONENTS_MAX_CLASSES:
        raise ValueError(f"{what}: needs 1..{COMPONENTS_MAX_CLASSES} classes, not {num_classes}")
    if int(H) < 1 or int(W) < 1 or int(H) * int(W) >= 1 << 31:
        raise ValueError(f"{what}: needs an image of at least 1x1 and fewer than 2^31 pixels, not {H}x{W}")


def components_host(labels: np.ndarray, num_classes: int, rule: ComponentRule) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The restatements applied as ``Components`` applies the calls: class maps (n,H,W) uint8 -> ``(clean_labels (n,H,W) uint8,
    stats (n,C,2) uint32, removed (n,C) uint32)``."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    root, size, stats = components_reference(labels, num_classes, rule.connectivity)
    clean, removed = component_filter_reference(labels, root, size, num_classes, rule.pack(num_classes))
    return clean, stats, removed


def changed_pixels(clean: np.ndarray, argmax: np.ndarray) -> int:
    """The pixels of one image that the filter relabelled."""
    return int((np.asarray(clean) != np.asarray(argmax)).sum())


class Components:
    """``oct_components`` + ``oct_component_filter`` for up to ``batch`` images of one shape: ``(labels_u8)`` -- (n,H,W) uint8
    class maps on the device -> ``clean_labels`` (n,H,W) uint8, ``stats`` (n,C,2) int32 and ``removed`` (n,C) int32 (the bits
    are uint32) on the device, queued on the current stream.  The statistics are those of the INPUT map.  Workspace, roots and
    sizes are the object's own."""

    def __init__(self, batch: int, H: int, W: int, num_classes: int, rule: ComponentRule, device):
        import torch
        from .. import _hip
        self.B, self.H, self.W, self.C = int(batch), int(H), int(W), int(num_classes)
        check_components(self.C, self.H, self.W)
        self.rule = rule
        self.packed = rule.pack(self.C)
        nbytes = int(_hip.lib().oct_components_workspace_bytes(self.B, self.H, self.W))
        if not nbytes:
            raise _hip.OctError(f"oct_components does not support B={batch}, {H}x{W}")
        self.device = torch.device(device)
        shape = (self.B, self.H, self.W)
        self.root = torch.empty(shape, dtype=torch.int32, device=self.device)
        self.size = torch.empty(shape, dtype=torch.int32, device=self.device)
        self.labels = torch.empty(shape, dtype=torch.uint8, device=self.device)
        self.stats = torch.empty((self.B, self.C, 2), dtype=torch.int32, device=self.device)
        self.removed = torch.empty((self.B, self.C), dtype=torch.int32, device=self.device)
        self.ws = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        self.outs, self.geometry = (self.labels, self.stats, self.removed), (self.B, self.H, self.W, self.C)

    def __call__(self, labels_u8, labels=None, stats=None, removed=None):
        import ctypes
        import torch
        from .. import _hip
        _hip.expect(labels_u8, "labels", device=self.device, dtype=torch.uint8, shape=(None, self.H, self.W))
        n = labels_u8.shape[0]
        if not 1 <= n <= self.B:
            raise _hip.OctError(f"labels needs a count n in 1..{self.B}, not {n}")
        labels, stats = _hip.out_view(labels, self.labels, n, "clean labels"), _hip.out_view(stats, self.stats, n, "stats")
        removed = _hip.out_view(removed, self.removed, n, "removed")
        st = _hip.stream_ptr(self.device)
        _hip.call("oct_components", self.device, labels_u8.data_ptr(), n, self.H, self.W, self.C, self.rule.connectivity,
                  self.ws.data_ptr(), self.ws.numel(), self.root.data_ptr(), self.size.data_ptr(), stats.data_ptr(), st)
        _hip.call("oct_component_filter", self.device, labels_u8.data_ptr(), self.root.data_ptr(), self.size.data_ptr(), n,
                  self.H, self.W, self.C, ctypes.byref(self.packed), self.ws.data_ptr(), self.ws.numel(), labels.data_ptr(),
                  removed.data_ptr(), st)
        return labels, stats, removed

    @staticmethod
    def to_host(labels, stats, removed, first_image: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """Device tensors -> ``(clean_labels (n,H,W) uint8, stats (n,C,2) uint32, removed (n,C) uint32)`` on the host (waits for
        the stream)."""
        return (labels.cpu().numpy().copy(), stats.cpu().numpy().view(np.uint32).copy(),
                removed.cpu().numpy().view(np.uint32).copy())
