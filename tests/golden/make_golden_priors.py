#!/usr/bin/env python3
"""Store the reference's real prior files and its joint-limit table as fixtures under tests/golden/reference_priors/, so that
tests/test_real_prior_files_cpu.py runs on any checkout:

    python tests/golden/make_golden_priors.py REFERENCE_CHECKOUT        (or $SMALIFY_REFERENCE)

  <name>.pkl.gz      the walking-toy pose prior pickles (and the copy the reference ships for Windows), gzipped byte for byte
                     (mtime 0: the output is reproducible)
  unity_betas.npz    the unity shape prior, as shipped
  joint_limits.npz   min_values / max_values of the reference's LimitPrior (smal_fitter/priors/joint_limits_prior.py)

What is produced is data (the reference's data files and the values its code derives), never reference source."""
import gzip
import importlib.util
import os
import shutil
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_priors")
POSE_PRIORS = ("walking_toy_symmetric_pose_prior_with_cov_35parts.pkl", "walking_toy_symmetric_pose_prior_with_cov_35parts_WIN.pkl")


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("SMALIFY_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "data", "priors")):
        raise SystemExit("usage: make_golden_priors.py REFERENCE_CHECKOUT (a checkout of the reference with data/priors)")
    priors = os.path.join(ref, "data", "priors")
    os.makedirs(OUT, exist_ok=True)
    for name in POSE_PRIORS:
        with open(os.path.join(priors, name), "rb") as src, open(os.path.join(OUT, name + ".gz"), "wb") as dst:
            with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=dst, mtime=0) as z:
                shutil.copyfileobj(src, z)
    shutil.copyfile(os.path.join(priors, "unity_betas.npz"), os.path.join(OUT, "unity_betas.npz"))
    spec = importlib.util.spec_from_file_location("ref_joint_limits", os.path.join(ref, "smal_fitter", "priors", "joint_limits_prior.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lp = mod.LimitPrior()
    np.savez(os.path.join(OUT, "joint_limits.npz"), min_values=np.asarray(lp.min_values), max_values=np.asarray(lp.max_values))
    for f in sorted(os.listdir(OUT)):
        print(f, os.path.getsize(os.path.join(OUT, f)))


if __name__ == "__main__":
    main()
