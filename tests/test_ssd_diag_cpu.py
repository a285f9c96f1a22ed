"""reference.ssd_diag, the oracle of the fused intra-chunk kernel, against
the sequential recurrence in float64. Every row is a single chunk (l = Q),
where the carried state is zero and y_diag is the whole scan output, so the
oracle that judges the kernel cannot be wrong in the kernel's own way."""

import pytest
import torch

from fms_fsdp_amd import ops
from fms_fsdp_amd.ops import reference
from test_ssd_docmask_cpu import naive_ssd_reset, starts_to_doc_start


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("Q,h,g,p,n", [(64, 6, 2, 8, 16), (32, 4, 1, 16, 8)])
def test_ssd_diag_oracle_is_the_recurrence(Q, h, g, p, n, masked):
    torch.manual_seed(Q + masked)
    dd, b = torch.float64, 3
    x = torch.randn(b, Q, h * p, dtype=dd)
    dt = torch.randn(b, Q, h, dtype=dd) * 2
    B, C = torch.randn(b, Q, g * n, dtype=dd), torch.randn(b, Q, g * n, dtype=dd)
    dtb = torch.randn(h, dtype=dd)
    Alog = torch.linspace(-4.0, 1.4, h, dtype=dd)
    rows = [[0, 1, 2, Q // 2], [0, Q - 1], [0]] if masked else [[0]] * b
    start = starts_to_doc_start(rows, Q)
    dm = ops.doc_mask_from_starts(start) if masked else None

    dtf, dacs = reference.ssd_prep(dt.reshape(b * Q, h), dtb, Alog, Q)
    xdt, _ = reference.ssd_xdt(x.reshape(b * Q, h * p), dtf, dacs, h, p, Q, dm)
    got = reference.ssd_diag(C.reshape(b * Q, g * n), B.reshape(b * Q, g * n),
                             dacs, xdt, h, g, p, n, Q, doc_mask=dm)
    # the op itself sends tensors that are not on a GPU to the oracle
    assert torch.equal(ops.ssd_diag(C.reshape(b * Q, g * n),
                                    B.reshape(b * Q, g * n), dacs, xdt, h, g,
                                    p, n, Q, doc_mask=dm), got)
    ref = naive_ssd_reset(x.view(b, Q, h, p),
                          torch.nn.functional.softplus(dt + dtb, threshold=1e9),
                          -torch.exp(Alog), B.view(b, Q, g, n),
                          C.view(b, Q, g, n), start)
    torch.testing.assert_close(got.view(b, h, Q, p).permute(0, 2, 1, 3), ref,
                               rtol=1e-9, atol=1e-12)
