"""CPU: the oracle differentiates with respect to its pixels, and its pixel gradient equals the REFERENCE's `pixel_values.grad`
(tests/golden/pixel_grad.npz, written by tests/golden/make_golden_pixel_grad.py) at the tolerance test_oracle_golden.py holds the
parameter-gradient slices to. The GPU tests (test_pixel_grad_gpu.py) compare the model against this oracle."""
import numpy as np

import golden_util as gu
import pixel_grad_ref as pr


def test_oracle_pixel_gradient_matches_reference():
    g, cfg, sd, x, inp, lab, am, tt = pr.fixture_case()
    grad, loss = pr.oracle_tf_pixel_grad(x, sd, cfg, inp, lab, am, tt, gu.PAD)
    assert list(grad.shape) == g["grad_shape"].tolist() == [2, 2, 3, 96, 96]
    assert abs(loss - float(g["loss"])) < 1e-4
    assert gu.rel_rms(pr.at_index(grad, g), g["grad_values"]) < 2e-3
    norms = pr.image_norms(grad)
    assert norms[1, 1] == 0.0 and float(g["grad_image_norms"][1, 1]) == 0.0        # eval mode: the masked, zero-padded image gets no gradient
    np.testing.assert_allclose(norms, g["grad_image_norms"], rtol=2e-3)
    assert float((grad[0] != 0).float().mean()) > 0.99                             # dense
