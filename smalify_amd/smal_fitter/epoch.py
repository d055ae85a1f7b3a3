"""Bookkeeping of SMALFitter's epoch evaluation (SMALFitter(..., epoch_evaluation=True)): which batch ranges are windows of the
reference's partition (optimize_to_joints.py:119-120), and whether an evaluation of the whole sequence is still that of the
fitter's present state.  Plain torch on whatever device the tensors live on: nothing here touches the engine."""
from __future__ import annotations

import operator


class WindowPartition:
    """the reference's windows of a sequence of N frames: range(j, min(N, j + window)) for j = 0, window, 2 window, ..."""

    def __init__(self, num_frames, window):
        if num_frames <= 0 or window <= 0:
            raise ValueError("num_frames and window must be positive")
        self.num_frames, self.window = int(num_frames), int(window)
        self.num_windows = (self.num_frames + self.window - 1) // self.window

    def frames(self, w):
        return range(w * self.window, min(self.num_frames, (w + 1) * self.window))

    def window_of(self, batch_range):
        """index of the window `batch_range` is EXACTLY, or None: a part of a window, a range across two, another order"""
        try:
            br = [operator.index(i) for i in batch_range]
        except TypeError:
            return None
        if not br or br[0] < 0 or br[0] % self.window or br[0] >= self.num_frames:
            return None
        w = br[0] // self.window
        return w if br == list(self.frames(w)) else None

    def frame_windows(self):
        """window index of every frame"""
        return [n // self.window for n in range(self.num_frames)]


class StateKey:
    """What an evaluation depended on: tensors by identity AND version counter (every in-place write bumps it: optimizer.step(),
    `target_visibility *= 0`, an item assignment), scalars by value.  The key holds the tensors themselves, so that the id of a
    freed tensor cannot come back as another one's.  requires_grad is not part of it: flipping it changes no value."""

    def __init__(self, tensors, scalars):
        self.tensors = tuple(tensors)
        self.versions = tuple(t._version for t in self.tensors)
        self.scalars = tuple(scalars)

    def matches(self, tensors, scalars):
        tensors = tuple(tensors)
        return (len(tensors) == len(self.tensors) and all(a is b for a, b in zip(tensors, self.tensors))
                and tuple(t._version for t in tensors) == self.versions and tuple(scalars) == self.scalars)
