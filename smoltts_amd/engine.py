"""The engine's names in one place, as they were before the module was split: a façade of re-exports and nothing else.

The code lives in ``abi`` (the ctypes binding of include/smoltts_hip.h), ``device`` (memory and stream helpers), ``lm`` (DualAR
engine, session, prefixes), ``mimi`` (codec), ``stages`` (the post-codec stages) and ``route`` (a stream's path through them).
Product modules import from those; tests and tools may keep importing from here.  Patching a name here does not reach the
module that uses it: patch it where it lives.
"""
from . import abi
from .abi import *  # noqa: F401,F403
from .device import *  # noqa: F401,F403
from .device import _UPLOAD_STREAMS, _alloc_slab, _require_gpu  # noqa: F401
from .lm import *  # noqa: F401,F403
from .lm import _fill_block  # noqa: F401
from .mimi import *  # noqa: F401,F403
from .route import *  # noqa: F401,F403
from .stages import *  # noqa: F401,F403
from .stages import _loudness_whole, _Stage, _whole_row  # noqa: F401

_EXPORTS = exported_symbols()  # noqa: F405


def __getattr__(name):  # the binding's own state (``_lib``) is read where it lives, never copied
    return getattr(abi, name)
