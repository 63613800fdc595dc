"""Record ``PoolMixtureMaker.draw`` of a fixed small pool into tests/golden/pool_draws.json.

The file was written by the commit BEFORE the maker learnt colouring, LTAS matching and BRIR decay: with those
options at their defaults the draws must stay what they were, and tests/test_mixture_fx_host.py holds them to this
record. Regenerating it on a later commit only records that commit against itself.

    python tests/golden/make_pool_draws.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]


def main():
    from brever_amd import mixture
    from mixture_fx_ref import DRAW_CONFIGS, DRAWS, draw_pool
    out = {}
    for name, kw in DRAW_CONFIGS.items():
        maker = mixture.PoolMixtureMaker(None, ['mixture'], 12, **kw, **draw_pool())
        out[name] = {str(epoch): maker.draw(epoch) for epoch in (0, 3)}
    with open(DRAWS, 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(DRAWS, os.path.getsize(DRAWS), 'bytes')


if __name__ == '__main__':
    main()
