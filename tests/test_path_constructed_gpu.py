"""fsdp_path_batch on the inputs of tests/path_support.py (a case at every branch of the path stage, a pair of cases 1e-9 either side of
every threshold), against the oracle in det mode: the four pinned forms of the stage (test_polyline_capacity.FORMS) and the exact
route (always_route), standard and wide build.  Family E and the tables of family F go through the context's global path.

One launch per (form, parameter set, global path).  The bar is the one every GPU comparison of the path stage here holds: status,
path_fallback, n_dense and the NaN rows equal, the path within 1e-9 of the oracle; the measured maximum is printed (0.0 is what the
other files measure).

Left to the emulator (tests/test_path_constructed_cpu.py), because they raise and the kernel source does not show at a glance that
every intermediate stays inside its arrays with such input: centres that are NaN or infinite, tracks at 1e17 m, a caller's previous
path that raises as well (path_support.Case.gpu False).  The cases that raise on an index (status 104) do go to the device: the
kernel tests j against [0, n) before it loads (path_front), and the counts stay within MAX_MATCH.

Run with -m gpu on an MI355X."""
import importlib
import time

import numpy as np
import pytest

import path_support as ps
from test_polyline_capacity import FORMS

pytestmark = pytest.mark.gpu

ROUTES = {**{k: v[0] for k, v in FORMS.items()}, "exact": {"path_mode": 2, "pack": 2, "fit_g": 4, "always_route": 1}}


@pytest.fixture(scope="module")
def pkg():
    return importlib.import_module("ft-fsd-path-planning_amd")


@pytest.fixture
def contexts(pkg):
    """one context per parameter set of the cases (a dozen), closed when the test ends"""
    made = {}

    def get(build, route, prm):
        key = (build, route, tuple(sorted(prm.items())))
        if key not in made:
            made[key] = pkg.Context(device=0, mission=int(pkg.MissionTypes.trackdrive), params=dict(prm) or None, shapes=pkg.WIDE if build == "wide" else None,
                                    options={"plan_chunks": 1, **ROUTES[route]})
            assert (made[key].shapes is pkg.WIDE) == (build == "wide")
        return made[key]

    yield get
    for c in made.values():
        c.close()


@pytest.mark.parametrize("build", ["standard", "wide"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_path_batch_on_constructed_inputs(contexts, build, route):
    wide = build == "wide"
    o, _ = ps.libs(wide)
    worst, n, t0 = 0.0, 0, time.perf_counter()
    for family, (cases, _pairs) in ps.everything(wide).items():
        rows, recs = ps.reference(wide)[family]
        keep = [i for i, c in enumerate(cases) if c.gpu]
        assert len(keep) >= 0.8 * len(cases)
        sub = [cases[i] for i in keep]
        want = ps.expected(rows, recs)[keep]
        n_dense = np.array([int(recs[i]["n_dense"]) if s == 0 else 0 for i, s in zip(keep, want["status"])])
        got = ps.run_gpu(lambda prm: contexts(build, route, prm), o, sub)
        if family == "C":  # (one launch, default parameters, no global path) the form ran the kernel it is named after
            names = contexts(build, route, {}).stage_names()
            assert ("path_retry_kernel" if route == "exact" else FORMS[route][1]) in names, names
        bad = np.flatnonzero(got["status"] != want["status"])
        assert len(bad) == 0, (family, [(sub[i].name, int(got["status"][i]), int(want["status"][i])) for i in bad[:6]])
        ok = want["status"] == 0
        bad = np.flatnonzero(ok & (got["path_fallback"] != want["path_fallback"]))
        assert len(bad) == 0, (family, [(sub[i].name, int(got["path_fallback"][i]), int(want["path_fallback"][i])) for i in bad[:6]])
        assert np.array_equal(got["n_dense"], n_dense), (family, [sub[i].name for i in np.flatnonzero(got["n_dense"] != n_dense)[:6]])
        assert np.array_equal(np.isnan(got["path"]), np.isnan(want["path"])), family
        err = np.nan_to_num(np.abs(got["path"] - want["path"]), nan=0.0).reshape(len(sub), -1).max(axis=1)
        assert (err <= 1e-9).all(), (family, [(sub[i].name, float(err[i])) for i in np.flatnonzero(err > 1e-9)[:6]])
        worst, n = max(worst, float(err.max())), n + len(sub)
    print(f"path_batch, {build} build, {route}: {n} cases, max |path - oracle| = {worst:.3e}, {time.perf_counter() - t0:.2f} s")
