"""Fixture conv_bwd_routes.json: the launch trace (tests/conv_route_trace.py) of every ConvBlock case, as issued by the package of
the checkout given -- a worktree of the commit whose routes are to be pinned: the one BEFORE a change to functional.Conv3x3Fn.
    python tests/golden/gen_conv_bwd_routes.py [CHECKOUT]          (default: this checkout)
Distinct calls and distinct traces are stored once: "calls" holds [name, arguments, result], "traces" lists of indices into it,
"cases" the index of the trace of each case of conv_route_trace.cases(), in its order."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import conv_route_trace as T  # noqa: E402


def rows(items, per_line):
    lines = [",".join(json.dumps(v, separators=(",", ":"), sort_keys=True) for v in items[i:i + per_line]) for i in range(0, len(items), per_line)]
    return "[\n" + ",\n".join(lines) + "\n]"


def main():
    calls, traces, cases = {}, {}, []
    for c in T.cases():
        tr = tuple(calls.setdefault(json.dumps(e, sort_keys=True), len(calls)) for e in T.run_case(c))
        cases.append(traces.setdefault(tr, len(traces)))
    path = os.path.join(HERE, "conv_bwd_routes.json")
    with open(path, "w") as f:
        f.write('{"calls":' + rows([json.loads(k) for k in calls], 1) + ',\n"traces":' + rows([list(t) for t in traces], 1) + ',\n"cases":' + rows(cases, 64) + "}\n")
    print(f"wrote {path} from {os.path.dirname(T.Fn.__file__)}: {len(cases)} cases, {len(traces)} traces, {len(calls)} calls, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
