"""Stand-in for the `rlp` package, enough for the reference's state/ modules to import and run
(tests/golden/make_state_golden.py): RLP of byte strings and nested lists, and the three sedes names
state/util/utils.py imports. Golden generation only; nothing in the package or the tests imports it."""
from . import codec, sedes  # noqa: F401
from .codec import decode, encode, encode_raw  # noqa: F401
