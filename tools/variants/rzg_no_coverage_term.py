"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): the coverage's derivative left out, Pu =
g_l sum_k q_k dt_k/dfu: a matte that moves with its layer is taken to stand still."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip",
    'const double Pu = el * au + gl * Cu, Pv = el * av + gl * Cv;',
    'const double Pu = gl * Cu, Pv = gl * Cv;')
