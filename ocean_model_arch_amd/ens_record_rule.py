"""The station recorder's schedule in Python (include/ocn_sw.h ocn_ens_record_due, ocn_ens_step_record): which
steps of a call write a record.  Pure Python: no device, no library.

A recorder counts the steps of its step_record() calls.  After the counted step (r + 1) * every it writes
record r, so a call of `nsteps` steps made after `counted` counted steps writes a record after each of its
1-based steps s with (counted + s) % every == 0.
"""
from __future__ import annotations

MAX_SERIES_BYTES = 1 << 30   # max_records x nobs x n doubles


def check(every: int, max_records: int) -> None:
    """ValueError as ocn_ens_record_begin refuses them."""
    if every < 1:
        raise ValueError(f"record: every = {every} < 1")
    if max_records < 1:
        raise ValueError(f"record: max_records = {max_records} < 1")


def due(counted: int, nsteps: int, every: int) -> list[int]:
    """The 1-based steps of a call at which a record is due, in rising order."""
    if counted < 0 or nsteps < 0 or every < 1:
        raise ValueError(f"due: counted = {counted}, nsteps = {nsteps}, every = {every}")
    return [s for s in range(1, nsteps + 1) if (counted + s) % every == 0]
