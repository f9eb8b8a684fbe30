"""Writes tests/golden/obsvec_runner_case5.npz: observation vectors the reference recorded with its Runner on rte_case5_example
(grid2op/data_test/runner_data/res_agent_<version>/{00,01}/observations.npz + episode_meta.json, data the reference ships for its own
backward-compatibility tests).  Every version whose vectors have the width of the current CompleteObservation on that grid (192) is taken;
per episode: the non-NaN rows (the reset observation, the played steps, the game-over observation when the episode ended early), the
number of played steps (nb_timestep_played: it counts the step that ended the episode) and the start time (the calendar columns of its first row).

    python tests/golden/make_obsvec_fixtures.py /path/to/reference/checkout
"""
import glob
import json
import os
import sys

import numpy as np

WIDTH = 192


def main(ref):
    base = os.path.join(ref, "grid2op", "data_test", "runner_data")
    vec, ep_of_row, played, start, names = [], [], [], [], []
    for d in sorted(glob.glob(os.path.join(base, "res_agent_*"))):
        for ep in ("00", "01"):
            p = os.path.join(d, ep, "observations.npz")
            if not os.path.exists(p):
                continue
            a = np.load(p)["data"]
            if a.ndim != 2 or a.shape[1] != WIDTH:
                continue
            rows = a[~np.isnan(a).all(axis=1)]
            with open(os.path.join(d, ep, "episode_meta.json")) as f:
                meta = json.load(f)
            ep_of_row += [len(names)] * len(rows)
            vec.append(rows.astype(np.float32))
            played.append(int(meta["nb_timestep_played"]))
            start.append(rows[0, :5].astype(np.int32))          # year, month, day, hour, minute
            names.append(os.path.basename(d)[len("res_agent_"):] + "/" + ep)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "obsvec_runner_case5.npz")
    np.savez_compressed(out, vectors=np.concatenate(vec), episode=np.asarray(ep_of_row, np.int32), played=np.asarray(played, np.int32),
                        start=np.stack(start), names=np.asarray(names))
    print(out, np.concatenate(vec).shape, names)


if __name__ == "__main__":
    main(sys.argv[1])
