"""What a SweepEngine knows about one launch block: the row list of each kernel, the class items, the owned plan and
where each of them puts its delta partials.  Data only: the launches that read it are in engine.py.  The records are
NamedTuples in the positional order their readers outside the engine unpack (``eng.class_rows[i]`` ...)."""
from __future__ import annotations

import itertools
from dataclasses import dataclass
from typing import NamedTuple, Optional

import numpy as np
import torch


class ClassItems(NamedTuple):
    """The class pass over some class rows (deg > class_threshold) of a block: the rows and xcd.class_items' work items,
    on the device."""
    rows: torch.Tensor              # int32, relative to the block's first row
    slot_ptr: torch.Tensor          # int64 [rows + 1]; slot_ptr[-1] is known on the host (BlockRows.n_slots)
    e0: torch.Tensor
    len: torch.Tensor
    slot: torch.Tensor
    row: torch.Tensor
    items_per_block: int

    @classmethod
    def upload(cls, items: dict, rows: np.ndarray, device) -> "ClassItems":
        """`items`: what xcd.class_items returned for `rows`."""
        up = lambda name: torch.from_numpy(items[name]).to(device)                         # noqa: E731
        return cls(torch.from_numpy(rows.astype(np.int32)).to(device), up("slot_ptr"), up("e0"), up("len"), up("slot"),
                   up("row"), items["items_per_block"])


class SplitRows(NamedTuple):
    """Rows above SPLIT_EDGES that are nobody's class rows, cut into segments: on the device."""
    rows: torch.Tensor
    seg_ptr: torch.Tensor
    seg_row: torch.Tensor


class OwnedRows(NamedTuple):
    """A block's class rows divided between the owned pass and chunk + combine (owned.plan_block)."""
    plan: object                    # the backend's plan of the rows of at most owned_max_edges edges
    rest: Optional[ClassItems]      # the class rows above them, None without any
    n_rest: int


@dataclass(frozen=True)
class PartialLayout:
    """Where the launches of one block put their delta partials, as starts relative to the block's first slot:

        [row pass | 4-wave rows | 16-wave rows | split rows | class rows]

    one slot per listed row, in list order.  With an owned pass the class rows' slots are [rows above | owned rows];
    both launches get the view at `klass`, so nothing here depends on that division."""
    main: int
    mid: int
    hub: int
    split: int
    klass: int
    end: int                        # the block's length

    @classmethod
    def of(cls, row_pass: int, n_mid: int, n_hub: int, n_split: int, n_class: int, length: int) -> "PartialLayout":
        """`row_pass`: slots of the one-(sub-)wave pass, spmm_partials_len(nrows, 0); `length`: what the backend sizes
        the block at, spmm_partials_len(nrows, long rows) -- which must be where this order ends."""
        starts = list(itertools.accumulate((row_pass, n_mid, n_hub, n_split, n_class), initial=0))
        assert starts[-1] == length, (starts, length)
        return cls(*starts)

    def owned(self, n_rest: int) -> int:
        """Start of the owned rows' slots when `n_rest` class rows stay on chunk + combine."""
        return self.klass + n_rest

    def owned_slots(self, n_rest: int, n_owned: int) -> np.ndarray:
        """The owned rows' slots relative to `klass` (an owned plan's row_part): however the class rows are divided,
        they fill the class region."""
        assert self.owned(n_rest) + n_owned == self.end, (self, n_rest, n_owned)
        return self.owned(n_rest) - self.klass + np.arange(n_owned)


@dataclass
class BlockRows:
    """One launch block.  Row lists are int32 on the device, relative to the block's first row (the kernels get rowptr /
    X / Z_new offset to it); None where no row qualifies."""
    long: Optional[torch.Tensor]        # every row above score_threshold (K2 slices these)
    k1_long: Optional[torch.Tensor]     # K1's workgroup-per-row list: above k1_threshold, not class
    mid: Optional[torch.Tensor]         # long_threshold < deg <= hub_threshold: 4 waves/row
    hub: Optional[torch.Tensor]         # hub_threshold < deg <= SPLIT_EDGES: 16 waves/row
    partials: PartialLayout
    split: Optional[SplitRows] = None   # deg > SPLIT_EDGES
    klass: Optional[ClassItems] = None  # deg > class_threshold
    n_slots: int = 0                    # klass.slot_ptr[-1], known on the host
    owned: Optional[OwnedRows] = None   # class_owned: how `klass` is divided; set_owned() replaces it
    owned_inputs: Optional[tuple] = None    # what owned.plan_block plans from, kept where an owned pass is possible
