"""Epsilon schedule of the reference trainer (src/scheduler.py): ``value(t) = a * exp(b * t)`` from ``value_from`` at step 0 to
``value_to`` at step ``num_steps - 1``, constant outside."""
from __future__ import annotations

import numpy as np


class ExponentialSchedule:
    def __init__(self, value_from: float, value_to: float, num_steps: int):
        self.value_from, self.value_to, self.num_steps = value_from, value_to, num_steps
        self.a = value_from
        self.b = np.log(value_to / value_from) / (num_steps - 1)

    def value(self, step) -> float:
        if step < 1:
            return self.value_from
        if step >= self.num_steps:
            return self.value_to
        return self.a * np.exp(self.b * step)
