"""The checks of a full-size output against a full-size golden stored in the layout of tests/golden/make_goldens.py's g12 /
g19: ``out_sub`` = y[:, :, 3::8, 5::16], ``out_rows`` = the first and the last full row, per-channel mean / square mean and
``abs_max``.  Shared by the fusion (g12 / g13 / g18) and the PointPillar encoder (g19) tests."""
import torch


def _rows(y):
    return [0, y.shape[2] - 1]


def full_size_report(g, y):
    """Error statistics of a full-size output against a full-size golden (sub-grid of every channel + first / last row):
    rel-max, rms-relative and the 99.9-percentile of the element-wise relative error |d| / max(|ref|, 1e-3 rms ref) -
    the last one is what bounds small-magnitude outputs, which a max-norm cannot see."""
    ref = torch.cat([g["out_sub"].flatten(), g["out_rows"].flatten()]).double()
    got = torch.cat([y[:, :, 3::8, 5::16].flatten(), y[:, :, _rows(y), :].flatten()]).double()
    d = (got - ref).abs()
    rms = ref.pow(2).mean().sqrt()
    elem = d / ref.abs().clamp_min(1e-3 * rms)
    k = max(1, int(round(0.999 * elem.numel())))
    return dict(rel_max=float(d.max() / float(g["abs_max"])), rms_rel=float(d.pow(2).mean().sqrt() / rms),
                p999=float(elem.kthvalue(k).values))


def check_full_size(g, y, tol, tag="", p999=None):
    """Sub-grid and both rows at rel-max `tol`, rms-relative at `tol`, p99.9 at `p999` (default 10 tol), channel mean at `tol`
    of the output's max and channel square mean at 2 tol of its largest; prints the figures as ``full-size[tag]``."""
    scale = float(g["abs_max"])
    e = full_size_report(g, y)
    print(f"\nfull-size[{tag}] rel-max {e['rel_max']:.2e} rms-rel {e['rms_rel']:.2e} p99.9 {e['p999']:.2e}")
    assert float((y[:, :, 3::8, 5::16] - g["out_sub"]).abs().max()) / scale < tol
    assert float((y[:, :, _rows(y), :] - g["out_rows"]).abs().max()) / scale < tol
    assert e["rms_rel"] < tol                   # rms-relative at the same bound as the max norm
    assert e["p999"] < (10 * tol if p999 is None else p999)
    y64 = y.double()
    assert float((y64.mean((0, 2, 3)) - g["chan_mean"]).abs().max()) / scale < tol
    assert float(((y64 * y64).mean((0, 2, 3)) - g["chan_sqmean"]).abs().max() / g["chan_sqmean"].max()) < 2 * tol
    return e
