"""numpy model of the observation stacks (include/imgenv.h, "observation stacks"): StateBatchWrapper's rule per robot.

    reset of the robot's world:  stack = [0, ..., 0, F]
    step:                        stack = [old[1], ..., old[K-1], F]

``F`` is the field's row of ``imgenv_out`` after the call; oldest first, newest last.  tests/test_stack_abi.py holds this model
to what the reference's own StateBatchWrapper returned (tests/golden/python_stack_*.npz); the GPU tests hold the library to it.
"""
import numpy as np


def depths(image_batch, state_batch, laser_batch, has_lasers=True):
    """effective depths (sensor_maps, vector_states, lasers) of the YAML keys (base.py:103-105); 0 = not stacked"""
    return (max(int(image_batch), 0), max(int(state_batch), 0), max(int(laser_batch), 1) if laser_batch >= 0 and has_lasers else 0)


class StackModel:
    """one field of depth ``k`` over ``n`` robots: ``value`` is ``[n, k, *frame]``"""

    def __init__(self, k):
        self.k, self.value = int(k), None

    def _value(self, frames):
        if self.value is None:
            self.value = np.zeros((frames.shape[0], self.k) + frames.shape[1:], frames.dtype)
        return self.value

    def reset(self, frames, rows):
        """a reset call: ``frames`` [n, ...] is the field after it, ``rows`` bool [n] the robots of the worlds it reset; the
        other robots' stacks stay as they are"""
        frames, rows = np.asarray(frames), np.asarray(rows, bool)
        v = self._value(frames)
        v[rows, :-1] = 0
        v[rows, -1] = frames[rows]
        return v

    def update(self, frames, reset_rows):
        """a step call: every robot's stack takes its frame; ``reset_rows`` bool [n]: robots whose world the call then reset
        (an auto-reset step; ``frames`` holds the new episode's first observation for them)"""
        frames = np.asarray(frames)
        v = self._value(frames)
        v[:, :-1] = v[:, 1:].copy()
        v[:, -1] = frames
        return self.reset(frames, reset_rows)


def bits(a):
    """the bit patterns of a float array (stacking only moves bytes: comparisons are exact, NaNs and signed zeros included)"""
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])
