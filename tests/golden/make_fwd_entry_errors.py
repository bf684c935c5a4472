"""Record tests/golden/fwd_entry_errors.json: status and sr_last_error() text of every case of tests/test_fwd_entries_host.py, from the
library that SATRENDER_LIB names (a build of the commit whose behaviour is to be kept), or the in-tree one.

    SATRENDER_LIB=build_variants/lib_parent.so python tests/golden/make_fwd_entry_errors.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import test_fwd_entries_host as T  # noqa: E402


def main():
    lib = T.load_lib()
    for entry in T.POINT + T.RENDER:
        assert T.call(lib, entry)[0] == 0, (entry, lib.sr_last_error().decode())
    rec = {}
    for entry, name, changes in T.CASES:
        status, error = T.call(lib, entry, changes)
        assert status != 0 and error, (entry, name, status, error)
        rec[T.case_id(entry, name)] = {"status": status, "error": error}
    assert len(rec) == len(T.CASES)
    with open(os.path.join(HERE, "fwd_entry_errors.json"), "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"recorded {len(rec)} cases")


if __name__ == "__main__":
    main()
