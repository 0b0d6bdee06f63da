"""The shared biquad-cascade models (tests/df2t_model.py): the numpy float32 loop is the oracle's section, bit for bit,
in both geometries the kernels run -- the equalizers' 14 bands x 4 sections and a CW filter's 1 x 6."""
import numpy as np

import cw_model
import df2t_model as M
import eq_model


def test_f32_loop_is_the_oracle_cascade(built):
    x = (0.25 * np.random.default_rng(41).standard_normal(512)).astype(np.float32)
    for coeffs in (eq_model.bands(), cw_model.tables()[0][3][None]):  # [14][4][5], [1][6][5]
        coeffs = np.ascontiguousarray(coeffs, np.float32)
        state = np.zeros(coeffs.shape[:2] + (2,), np.float32)
        want = np.stack([M.cascade_oracle(coeffs[b], state[b], x) for b in range(coeffs.shape[0])])
        got = M.cascade_f32(x, coeffs)
        assert got.shape == want.shape and np.abs(want).max() > 0 and np.abs(state).max() > 0
        assert np.array_equal(got, want)
