"""Writes tests/golden/id_maps.npz: the keys and values of one `user_dict` / `item_dict` pair that the reference saved next to its
checkpoints (recorded results; every saved pair is identical, which this script checks before it writes).

    python tools/make_id_maps_golden.py <directory with user_dict_*.pkl and item_dict_*.pkl, searched recursively>

The arrays hold no pickled objects: user keys as fixed-width unicode, everything else int64."""
import glob
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(src: str) -> None:
    pairs = {}
    for kind in ("user", "item"):
        dicts = []
        for path in sorted(glob.glob(os.path.join(src, "**", f"{kind}_dict_*.pkl"), recursive=True)):
            with open(path, "rb") as f:
                dicts.append(pickle.load(f))
        if not dicts:
            raise SystemExit(f"no {kind}_dict_*.pkl under {src}")
        first = list(dicts[0].items())
        assert all(list(d.items()) == first for d in dicts), f"the saved {kind} dictionaries differ"
        pairs[kind] = (first, len(dicts))
    users, n_u = pairs["user"]
    items, n_i = pairs["item"]
    out = os.path.join(ROOT, "tests", "golden", "id_maps.npz")
    np.savez_compressed(out, user_keys=np.array([k for k, _ in users], dtype=str), user_ids=np.array([v for _, v in users], dtype=np.int64),
                        item_keys=np.array([int(k) for k, _ in items], dtype=np.int64), item_ids=np.array([v for _, v in items], dtype=np.int64))
    print(f"{out}: {len(users)} users ({n_u} identical dictionaries), {len(items)} items ({n_i}), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main(sys.argv[1])
