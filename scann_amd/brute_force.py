"""The dataset of the exact brute-force searcher (score_brute_force()
without a tree): what smx_bf_create uploads."""
from __future__ import annotations

import ctypes
import dataclasses

import numpy as np

from .index import METRIC_DOT, METRIC_SQUARED_L2


class BruteForceDesc(ctypes.Structure):
    """ctypes mirror of smx_bf_desc."""

    _fields_ = [("metric", ctypes.c_int32), ("dim", ctypes.c_int32),
                ("num_datapoints", ctypes.c_uint32), ("reserved", ctypes.c_int32),
                ("dataset", ctypes.c_void_p)]


@dataclasses.dataclass
class BruteForceIndex:
    dataset: np.ndarray     # float32 [N][dim], C order
    metric: int             # METRIC_DOT | METRIC_SQUARED_L2

    def __post_init__(self):
        self.dataset = np.ascontiguousarray(self.dataset, dtype=np.float32)
        if self.dataset.ndim != 2:
            raise ValueError("dataset must be two-dimensional")
        if self.metric not in (METRIC_DOT, METRIC_SQUARED_L2):
            raise ValueError(f"unknown metric {self.metric!r}")

    @property
    def num_datapoints(self) -> int:
        return int(self.dataset.shape[0])

    @property
    def dim(self) -> int:
        return int(self.dataset.shape[1])

    def desc(self) -> BruteForceDesc:
        """Borrowed-pointer descriptor; keep ``self`` alive while it is used."""
        return BruteForceDesc(metric=self.metric, dim=self.dim,
                              num_datapoints=self.num_datapoints, reserved=0,
                              dataset=self.dataset.ctypes.data)
