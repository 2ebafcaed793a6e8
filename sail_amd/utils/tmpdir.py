"""Per-user scratch directories under the system temp dir.

A fixed name such as <tmp>/sail_checkpoints belongs to whichever user
created it first; every other user on the machine then fails with
PermissionError. The user id in the name keeps them apart."""
from __future__ import annotations

import os
import tempfile


def user_tmp(name: str) -> str:
    """Path (not created) of this user's scratch directory `name`."""
    uid = os.getuid() if hasattr(os, "getuid") else 0
    return os.path.join(tempfile.gettempdir(), f"{name}-{uid}")
