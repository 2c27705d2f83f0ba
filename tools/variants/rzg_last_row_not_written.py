"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): the last workgroup writes no row."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    '    if ((int)threadIdx.x < comps) {\n        double v = 0.0;',
    '    if ((int)threadIdx.x < comps && blockIdx.x + 1 < gridDim.x) {\n        double v = 0.0;')
