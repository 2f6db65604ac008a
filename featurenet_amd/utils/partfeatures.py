"""The features of generated parts as records: one :class:`PartFeature` per used row of a
parameter table (``ops.partgen``), the ground truth that goes with the label volume.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

FACES = ("+z", "-z", "+x", "-x", "+y", "-y")


@dataclass
class PartFeature:
    """One feature of one part."""
    slot: int                # its row in the part's table; the label volume's ``slots`` holds slot + 1
    cls: int                 # its class, 0..23; the label volume holds cls + 1
    orientation: int         # o + 6 fx + 12 fy: access face o (FACES), canonical x / y mirrored
    bbox: tuple              # (z0, y0, x0, z1, y1, x1), bounds inclusive, as FeatureInstance.bbox

    @property
    def face(self) -> str:
        return FACES[self.orientation % 6]

    def to_dict(self) -> dict:
        """JSON-safe record."""
        return {"slot": self.slot, "class": self.cls, "orientation": self.orientation, "face": self.face,
                "bbox": list(self.bbox)}


def from_params(params) -> "list[list[PartFeature]]":
    """Per-part record lists from a parameter table int32 ``[N, K, 16]`` (tensor or array)."""
    tab = np.asarray(params.cpu() if hasattr(params, "cpu") else params, dtype=np.int64)
    if tab.ndim != 3 or tab.shape[2] != 16:
        raise ValueError(f"from_params: params must be [N, K, 16], not {tab.shape}")
    out = []
    for part in tab:
        out.append([PartFeature(slot=k, cls=int(row[0]), orientation=int(row[1]),
                                bbox=(int(row[14]), int(row[12]), int(row[10]), int(row[15]), int(row[13]),
                                      int(row[11])))
                    for k, row in enumerate(part) if row[0] >= 0])
    return out
