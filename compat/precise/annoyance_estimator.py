"""Opt-in literal-name alias (put `<repo>/compat` on sys.path): `precise.annoyance_estimator` IS `mycroft_precise_amd.annoyance`.
Not a component: one line that hands the import system the MI355X module under the reference's module name
(`precise/annoyance_estimator.py`), so that `from precise.annoyance_estimator import AnnoyanceEstimate` resolves to this
framework; the estimate itself is `annoyance.estimate`, over bucket arrays counted on the device."""
import sys
import mycroft_precise_amd.annoyance as _impl

sys.modules[__name__] = _impl
