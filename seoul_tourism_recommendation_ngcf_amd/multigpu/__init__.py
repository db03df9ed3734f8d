"""The code behind `dist` (whose docstring is the design note): one module per concern, imported by `dist.py`, nothing here."""
