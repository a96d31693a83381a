"""A child process of tests/test_gpu_pair_wide.py::test_the_other_forms_of_the_passes (not a test: pytest does not collect
it).  The library reads FPIC_PAIR_FORMS once per process, so the parent starts this script afresh for every value; it
computes the digests of the wide scenes (test_gpu_pair_wide.digests) under the forms its environment selects and prints them
as one line of JSON."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "fusion-sim_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import fusionpic
    import test_gpu_pair_wide as wide_tests
    fusionpic.load_library()
    print(json.dumps(dict(forms=os.environ.get("FPIC_PAIR_FORMS", "default"), digests=wide_tests.digests(fusionpic))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
