"""The hostsim à-trous filter's bits, pinned: rt_denoise and rt_denoise_var over test_denoise.SIZES x guides on and
off x passes 1..5 at blend 0.75 and the default sigmas, on the inputs test_denoise.synth() and dnv_cases.inputs()
produce (the sigma map's NaN and +inf entries included), sigma_out asked for. A case's result is the SHA-256 of
each output's bytes.

Shared by tools/gen_golden_atrous_bits.py, which records tests/golden/atrous_bits.json, and
tests/test_atrous_bits.py, which recomputes the digests and compares.

Helpers only: no tests here."""
from __future__ import annotations

import hashlib
import os

import dnv_cases as dv
import test_denoise as dn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "atrous_bits.json")
BLEND = 0.75
PASSES = (1, 2, 3, 4, 5)
CASES = [(w, h, passes, guides) for (w, h) in dn.SIZES for passes in PASSES for guides in (True, False)]


def key(w, h, passes, guides):
    return f"{w}x{h}/passes{passes}/{'guides' if guides else 'colour'}"


def _sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def digests(w, h, passes, guides):
    """{output name: digest} of one case, from the hostsim results the other tests share."""
    rgba_var, sigma_out = dv.host_result(w, h, passes, guides, BLEND)
    return {"denoise": _sha(dn.host_result(w, h, passes, guides, BLEND)), "denoise_var": _sha(rgba_var),
            "denoise_var_sigma_out": _sha(sigma_out)}


def run_all():
    return {key(*c): digests(*c) for c in CASES}
