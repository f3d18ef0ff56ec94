"""the real-text fixture of tests/test_host.py::test_data_prep_iac_on_the_reference_posts: the `post` column of the reference's
docs/results_iac/clustering.csv (1 901 cleaned IAC posts, the only corpus the reference tree holds), in csv order and unchanged,
as a JSON list of strings compressed with xz -> tests/golden/iac_posts.json.xz.  Data only: no reference code.

    python tests/golden/make_iac_posts_golden.py <reference tree>/docs/results_iac/clustering.csv"""
import csv
import json
import lzma
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))

csv.field_size_limit(1 << 30)
with open(sys.argv[1], newline='') as f:
    posts = [r['post'] for r in csv.DictReader(f)]
with lzma.open(os.path.join(HERE, 'iac_posts.json.xz'), 'wb', preset=9) as f:
    f.write(json.dumps(posts, ensure_ascii=False).encode('utf-8'))
print(len(posts), 'posts')
