"""Generates tests/golden/defaultparms.yaml: the values of the reference's stock parameter file (prisim/examples/simparms/defaultparms.yaml),
parsed and written back without its comments, so that tests/test_driver.py loads what the reference ships without the reference tree.

  python tests/golden/make_defaultparms.py <reference checkout>/prisim/examples/simparms/defaultparms.yaml
"""
import os
import sys

import yaml

HERE = os.path.dirname(os.path.abspath(__file__))


def main(src):
    with open(src) as f:
        parms = yaml.safe_load(f)
    text = yaml.safe_dump(parms, default_flow_style=False, sort_keys=True)
    if yaml.safe_load(text) != parms:
        raise SystemExit('the values do not survive the round trip')
    with open(os.path.join(HERE, 'defaultparms.yaml'), 'w') as f:
        f.write('# Values of the reference\'s prisim/examples/simparms/defaultparms.yaml (tests/golden/make_defaultparms.py)\n')
        f.write(text)


if __name__ == '__main__':
    main(sys.argv[1])
