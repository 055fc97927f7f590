"""CPU, build container only (skipped where oracle/_ref is not built): the expectation tests/test_gpu_residual_estimate.py
leans on — orc.residual_records -> orc.estimate_records_from — pinned once more to the compiled reference end to end.  For random
blocks the reference's own records of the block, costed by the reference's BitEstimator_Std whose contexts were assigned from a
coder that had adapted over a history, equal the oracle composition from the states that call reports.  So a wrong expectation
cannot hide behind the device agreeing with itself."""
import numpy as np
import pytest

import helpers as H

needs_ref = pytest.mark.skipif(not H.ref_available(), reason="oracle/_ref not built (reference sources are in the build container only)")

SIZES = [(4, 4), (8, 8), (16, 16), (32, 32), (64, 64), (2, 8), (8, 2), (16, 1), (1, 16), (4, 32), (64, 4), (16, 8)]
RES_POOL = np.concatenate([np.arange(86, 292), np.arange(310, 312), np.arange(357, 379)])


@needs_ref
@pytest.mark.parametrize("chroma", [0, 1])
def test_block_cost_from_adapted_contexts_matches_reference(chroma):
    orc, ref = H.load_oracle(), H.load_ref()
    rng = np.random.default_rng(0xE57 + chroma)
    for w, h in SIZES:
        for k in range(6):
            c = H.random_block(rng, w, h, density=[0.08, 0.5, 1.0][k % 3], big=[0.0, 0.1][k % 2], huge=0.02 if k == 5 else 0.0)
            flags = int(rng.integers(0, 8))
            want_rec, _ = ref.residual_records(c, chroma, flags)
            if max(w, h) > 32:
                flags &= ~H.TU_TS_FLAG          # TU::isTSAllowed is the caller's to evaluate
            hist = H.random_records(rng, int(rng.integers(0, 3000)), ctx_frac=0.9, ctx_pool=RES_POOL, end_trm=False)
            qp, iid = int(rng.integers(0, 64)), int(rng.integers(0, 3))
            rc, bits, s0, s1, rate = ref.estimate_from_history(hist, want_rec, qp, iid)
            assert rc == 0
            got_rec, _, _ = orc.residual_records(c, chroma, flags)
            assert orc.estimate_records_from(got_rec, s0, s1, rate) == (0, bits), (w, h, k, flags)


@needs_ref
def test_transform_skip_block_cost_matches_reference():
    orc, ref = H.load_oracle(), H.load_ref()
    rng = np.random.default_rng(0xE59)
    for w, h in [(4, 4), (8, 8), (32, 32), (2, 16), (16, 4)]:
        for k, extra in enumerate((H.TU_TS_FLAG, H.TU_BDPCM, 0)):
            c = (rng.integers(-6, 7, (h, w)) * (rng.random((h, w)) < 0.6)).astype(np.int32)
            c[0, 0] = 3
            flags = H.TU_TRANSFORM_SKIP | extra | (k & 3)
            want_rec, _ = ref.residual_records(c, k & 1, flags)
            hist = H.random_records(rng, 2000, ctx_frac=0.9, ctx_pool=RES_POOL, end_trm=False)
            rc, bits, s0, s1, rate = ref.estimate_from_history(hist, want_rec, 30, 1)
            assert rc == 0
            got_rec, _, _ = orc.residual_records(c, k & 1, flags)
            assert orc.estimate_records_from(got_rec, s0, s1, rate) == (0, bits), (w, h, flags)
