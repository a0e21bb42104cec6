"""--dump-outputs DIR: what the timed path computed in its last step, as .npy files two builds can be compared by."""
import os

import numpy as np

MAX_BYTES = 64 * 1000 * 1000          # all files together
SAMPLE_SEED = 20241015                # the rows kept when the whole output is larger than MAX_BYTES


def write_outputs(directory, call_id, logp, summary, max_bytes=MAX_BYTES):
    """Per call, in global call order: `call_id` (position in the workload's call order), `logp` (Viterbi log-probability) and
    `summary` (the 8 path-summary integers the engine returns), all float64 (the integers are exact).  When the three
    arrays exceed max_bytes, a fixed seeded sample of the calls is written (the same rows for the same number of calls).
    Returns {name: shape} of what was written."""
    call_id = np.asarray(call_id, np.int64)
    logp = np.asarray(logp, np.float64)
    summary = np.asarray(summary).reshape(len(call_id), -1)
    if not (len(call_id) == len(logp) == len(summary)):
        raise ValueError("write_outputs: %d ids, %d log-probabilities, %d summaries" % (len(call_id), len(logp), len(summary)))
    order = np.argsort(call_id, kind="stable")
    n = len(order)
    row_bytes = 8 * (2 + summary.shape[1])
    keep = max_bytes // row_bytes
    if n > keep:
        order = order[np.sort(np.random.default_rng(SAMPLE_SEED).choice(n, size=keep, replace=False))]
    os.makedirs(directory, exist_ok=True)
    arrays = {"call_id": call_id[order].astype(np.float64), "logp": logp[order],
              "summary": summary[order].astype(np.float64)}
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a))
    return {name: a.shape for name, a in arrays.items()}
