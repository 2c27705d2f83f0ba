"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): the back-to-front walk starts with R = 0
at the layer where T reached 0, as if the forward's walk had been kept: what lies behind an opaque texel is left out of R."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    '                R = R + cover * d;\n            }\n        }\n    }\n    block_sum_store_rows',
    '                R = Tl != 0.0 ? R + cover * d : 0.0;\n            }\n        }\n    }\n    block_sum_store_rows')
