#!/usr/bin/env python3
"""Record what the SpatialDQN entry points and wrappers answer to the tables of tests/spatial_desc_cases.py.

    python tests/golden/generate_spatial_refusals.py            # rewrites tests/golden/spatial_refusals.json

The committed spatial_refusals.json was written by this script AT THE PARENT of the commit that moved the spatial rules, the learners' shared
checks and the Python description of a served SpatialDQN into one place each: it holds the answers of the code BEFORE the move (every refusal's
return code and full susnet_last_error(), the wrappers' accept sets and spatial_unserved_reason's texts), and tests/test_spatial_desc_host.py
holds the moved code to them.  Run it again only when a message or an accept set is changed on purpose.  Needs the built library, no device;
only DATA is written."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import spatial_desc_cases  # noqa: E402

if __name__ == "__main__":
    path = os.path.join(HERE, "spatial_refusals.json")
    with open(path, "w") as f:
        json.dump(spatial_desc_cases.record(), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)
