"""The glue-fusion switch (see py_utils.GlueFusion for what it routes).

It lives under ops so that op wrappers can read it without importing core.
"""

_ENABLED = [True]


def enabled() -> bool:
  return _ENABLED[0]


def set_enabled(value: bool) -> bool:
  """Sets the switch; returns the previous value."""
  prev = _ENABLED[0]
  _ENABLED[0] = bool(value)
  return prev
