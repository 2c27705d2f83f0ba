"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): the adjoint of den dropped from A_side."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'A[side] = (double)r.ra * (sum + gd[side]);',
    'A[side] = (double)r.ra * sum;')
