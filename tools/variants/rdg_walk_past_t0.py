"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): the walk over the layers goes on behind T == 0 (the forward's stops
there): with finite textures the layers behind add exact zeros, with a non-finite one 0 x NaN."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '                if (Tn == 0.0) break;\n',
    '')
