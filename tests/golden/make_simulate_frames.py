"""Record what the reference's visualisation draws on mpcx's closed-loop arrays.

    python tests/golden/make_simulate_frames.py REFERENCE_DIR      (needs matplotlib)

Runs REFERENCE_DIR/simulation_code.py's ``simulate(cat_states, cat_controls, t, step_horizon, N,
reference)`` unchanged (matplotlib on the Agg backend; FuncAnimation replaced by a driver that
calls the script's init_func, then animate(i) and a full render for every frame) on the arrays of
tests/test_simulate.py's ``reference_loop_log`` and writes the data of the artists it draws to
tests/golden/simulate_frames.npz: numbers only, nothing of the script's text.

* ``path_x`` / ``path_y`` (frames, frames): the path line after frame i is row i's first i + 1 entries
  (NaN beyond);
* ``horizon`` (frames, 2, N + 1): the predicted-horizon line of frame i;
* ``vehicle`` (frames, 4, 2), ``target`` (4, 2): the polygons of the current and the target pose;
* ``xlim`` / ``ylim``: the axes' limits; ``frames``: how many frames the animation has;
* ``shape_cat_states`` / ``shape_cat_controls`` / ``shape_t``: the shapes of the arrays it accepted
  (all float64), ``step_horizon``, ``N``, ``reference``: the remaining arguments of the call.
"""
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "mpc-verde_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main(ref_dir):
    import matplotlib

    matplotlib.use("Agg", force=True)
    from matplotlib import animation

    from test_simulate import reference_loop_log

    rec = {"path": [], "horizon": [], "vehicle": [], "target": None, "xlim": None, "ylim": None}

    class EveryFrame:
        def __init__(self, fig=None, func=None, frames=None, init_func=None, **kw):
            if init_func is not None:
                init_func()
            for i in range(frames if isinstance(frames, int) else len(list(frames))):
                path, horizon, vehicle, target = func(i)
                fig.canvas.draw()
                rec["path"].append(np.array(path.get_data(), float))
                rec["horizon"].append(np.array(horizon.get_data(), float))
                rec["vehicle"].append(np.array(vehicle.get_xy(), float))
                rec["target"] = np.array(target.get_xy(), float)
            rec["xlim"], rec["ylim"] = fig.axes[0].get_xlim(), fig.axes[0].get_ylim()

    animation.FuncAnimation = EveryFrame
    spec = importlib.util.spec_from_file_location("simulation_code", os.path.join(ref_dir, "simulation_code.py"))
    sim = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sim)

    N, T = 10, 0.2
    log, _ = reference_loop_log(N, T)
    reference = np.array([0.0, 0.0, 0.0, 10.0, 10.0, 0.0])
    assert all(a.dtype == np.float64 for a in (log.cat_states, log.cat_controls, log.times))
    sim.simulate(log.cat_states, log.cat_controls, log.times, T, N, reference, save=False)
    n = len(rec["path"])
    px, py = np.full((n, n), np.nan), np.full((n, n), np.nan)
    for i, p in enumerate(rec["path"]):
        assert p.shape == (2, i + 1)
        px[i, :i + 1], py[i, :i + 1] = p
    np.savez_compressed(os.path.join(HERE, "simulate_frames.npz"), path_x=px, path_y=py,
                        horizon=np.array(rec["horizon"]), vehicle=np.array(rec["vehicle"]), target=rec["target"],
                        xlim=np.array(rec["xlim"], float), ylim=np.array(rec["ylim"], float), frames=np.array(n),
                        shape_cat_states=np.array(log.cat_states.shape), shape_cat_controls=np.array(log.cat_controls.shape),
                        shape_t=np.array(log.times.shape), step_horizon=np.array(T), N=np.array(N), reference=reference)
    print("wrote simulate_frames.npz:", n, "frames")


if __name__ == "__main__":
    main(sys.argv[1])
