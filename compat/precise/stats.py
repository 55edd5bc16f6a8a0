"""Opt-in literal-name alias (put `<repo>/compat` on sys.path): `precise.stats` IS `mycroft_precise_amd.stats`.
Not a component: one line that hands the import system the MI355X module under the reference's module name
(`precise/stats.py`), so unchanged reference-side code -- `from precise.stats import Stats` -- resolves to this framework."""
import sys
import mycroft_precise_amd.stats as _impl

sys.modules[__name__] = _impl
