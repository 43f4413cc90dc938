"""The work decompositions of csrc/conv2d_wino2.hip against the float64 reference (tests/conv2d_ref.py) at the route bound C_ROUTE["wino2"]
(8 x 2^-24 x A): every channel grouping (cout 32 / 96: the 8 x 16 x 32 items; 64 / 128 / 320 / 512: the 4 x 16 x 64 operand-reuse items), cin
32 .. 512, both dilations, ragged tile edges, the full PSM and ResNet shapes.  Each case runs through tests/test_gpu_conv2d_routes.py's
``run_case``: the instance that ran is asserted by name, both bindings and a raw C-ABI launch on NaN-guarded buffers agree bit for bit and
nothing outside the output is written."""
import pytest
import torch

import test_gpu_conv2d_routes as RT

pytestmark = pytest.mark.gpu

EDGE = [(1, 1, 1), (2, 5, 17), (1, 4, 16), (3, 9, 33), (1, 13, 47)]        # ragged 4- and 8-row tiles, partial column tiles


def _case(cid, shapes, cin, cout, dil, **kw):
    return RT.K(cid, "plan", "wino2", shapes, cin=cin, cout=cout, dil=dil, kern="conv2d_wino2_kernel<%d>" % dil, **kw)


CASES = []
for dil in (1, 2):
    for cin, cout in ((32, 32), (32, 64), (64, 96), (96, 128), (128, 320), (32, 512), (512, 64), (320, 128)):
        CASES.append(_case("edge-d%d-%d-%d" % (dil, cin, cout), EDGE, cin, cout, dil, rb=True, res=(cin + cout) % 3 == 0, ra=cout % 64 == 0))
CASES += [
    # the PSM feature extractor at 5 x 480 x 640 and the ResNet-50 layer1 block
    _case("full-psm-32", [(5, 240, 320)], 32, 32, 1, res=True),
    _case("full-psm-64", [(5, 120, 160)], 64, 64, 1, rb=True, res=True),
    _case("full-psm-128", [(5, 120, 160)], 128, 128, 1, res=True),
    _case("full-psm-128-dil2", [(5, 120, 160)], 128, 128, 2, res=True),
    _case("full-psm-320-128", [(5, 120, 160)], 320, 128, 1, rb=True),
    _case("full-resnet-layer1", [(5, 120, 160)], 64, 64, 1, ra=True),
    _case("full-resnet-layer4", [(5, 15, 20)], 512, 512, 1, ra=True),
]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (no CPU path exists)")


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_conv2d_wino2_decomposition_against_fp64(case):
    ratio, kernels = RT.run_case(case)
    assert kernels == [case["kern"]], kernels
    print("WINO2-RATIO %s %.3f" % (case["id"], ratio))
