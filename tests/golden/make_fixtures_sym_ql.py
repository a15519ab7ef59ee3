"""Writes tests/golden/sym_ql_model.json: the figures of the NumPy model of the Householder + QL eigensolver (tests/_sym_ql_model.py) for every
case of tests/test_gpu_sym_ql.py.  The device tests take their bounds from this record; tests/test_sym_ql_host.py repeats the cases up to order
301 live and compares.  The large cases take the model a minute or more each (the QL iteration is a Python loop), which is why they are recorded.

    python tests/golden/make_fixtures_sym_ql.py [--jobs N] [name ...]        (no name: every case; names: only those, merged into the record)
"""
import json
import multiprocessing
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import _sym_ql_model as M          # noqa: E402


def one(name):
    t0 = time.time()
    r = M.run_case(name)
    print(f"{name}: {time.time() - t0:.1f} s  {r}", flush=True)
    return name, r


def main(argv):
    jobs = 1
    if argv[:1] == ["--jobs"]:
        jobs, argv = int(argv[1]), argv[2:]
    path = M.record_path()
    out = M.recorded() if argv and os.path.exists(path) else {}
    names = argv or list(M.cases())
    names.sort(key=lambda n: -M.cases_order(n))          # (the long ones first)
    if jobs > 1:
        with multiprocessing.Pool(jobs) as pool:
            out.update(pool.imap_unordered(one, names))
    else:
        out.update(one(n) for n in names)
    with open(path, "w") as f:
        json.dump({k: out[k] for k in M.cases() if k in out}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
