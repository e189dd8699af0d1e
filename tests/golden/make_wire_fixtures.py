#!/usr/bin/env python3
"""Generates tests/golden/wire_fixtures.json - runs where a checkout of the reference exists (GRL_REFERENCE_DIR).

What it pins: wire.py's protobuf surface against the reference's committed stubs (python/generals_pb, imported here,
never copied) and its client (python/experience_stream_client.py: ExperienceStreamClient._process_experience).
  * schema: for every enum and message wire.py declares, the enum's value names and numbers and the message's field
    table (number -> name, type, repeated, message type, enum type, oneof), read from the reference's descriptors;
  * game_updates: the GameUpdates of tests/test_wire.py::_cross_parse_messages, parsed by the reference's stubs - their
    MessageToDict and their deterministic re-serialisation;
  * experience_batch: the same for the ExperienceBatch, plus what the reference's client decoded from its second
    experience (arrays as dtype / shape / flat list, scalars with their Python type).

Nothing of the reference travels: only this JSON does.  Consumer: tests/test_wire.py (CPU).

    GRL_REFERENCE_DIR=<checkout of the reference> python tests/golden/make_wire_fixtures.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("GRL_REFERENCE_DIR")
if not REF or not os.path.isdir(os.path.join(REF, "python", "generals_pb")):
    raise SystemExit("set GRL_REFERENCE_DIR to a checkout of the reference (python/generals_pb must exist)")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(REF, "python"))

from google.protobuf.json_format import MessageToDict  # noqa: E402

import test_wire as T  # noqa: E402
from experience_stream_client import ExperienceConfig, ExperienceStreamClient  # noqa: E402  (the reference's client)
from generals_pb.common.v1 import common_pb2  # noqa: E402  (the reference's committed stubs)
from generals_pb.experience.v1 import experience_pb2  # noqa: E402
from generals_pb.game.v1 import game_pb2  # noqa: E402


def encode_value(v):
    if isinstance(v, np.ndarray):
        data = [float(x) for x in v.ravel()] if v.dtype.kind == "f" else [bool(x) if v.dtype.kind == "b" else int(x) for x in v.ravel()]
        return {"dtype": str(v.dtype), "shape": list(v.shape), "data": data}
    return {"type": type(v).__name__, "value": v}


def main():
    mods = {"generals.common.v1": common_pb2, "generals.game.v1": game_pb2, "generals.experience.v1": experience_pb2}
    schema = {}
    for spec in T.wire._SCHEMA.values():   # what wire.py declares, as the reference's descriptors have it
        fd = mods[spec["package"]].DESCRIPTOR
        schema[spec["package"]] = {
            "enums": {n: [[v.name, v.number] for v in fd.enum_types_by_name[n].values] for n in spec["enums"]},
            "messages": {n: {str(k): list(v) for k, v in T._field_table(fd.message_types_by_name[n]).items()} for n in spec["messages"]}}
    ups, d, batch = T._cross_parse_messages()
    game_updates = []
    for up in ups:
        theirs = game_pb2.GameUpdate.FromString(up.SerializeToString())
        game_updates.append({"json": MessageToDict(theirs), "wire_hex": theirs.SerializeToString(deterministic=True).hex()})
    tb = experience_pb2.ExperienceBatch.FromString(batch.SerializeToString())
    back = ExperienceStreamClient(ExperienceConfig())._process_experience(tb.experiences[1])
    out = {"source": "recorded by tests/golden/make_wire_fixtures.py from the reference's python/generals_pb stubs and "
                     "python/experience_stream_client.py",
           "schema": schema, "game_updates": game_updates,
           "experience_batch": {"json": MessageToDict(tb), "wire_hex": tb.SerializeToString(deterministic=True).hex(),
                                "client_processed": {k: encode_value(v) for k, v in back.items() if k in d}}}
    path = os.path.join(HERE, "wire_fixtures.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {path}: {sum(len(p['messages']) for p in schema.values())} messages, {len(game_updates)} updates")


if __name__ == "__main__":
    main()
