"""k_render_layers_grad mutant (profiles/render_layers_grad/mutants.txt): the two views of gnum exchanged in q_k."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'qk[k] = ((double)ws[0] * (double)r.ra) * gn[0][k];',
    'qk[k] = ((double)ws[0] * (double)r.ra) * gn[V - 1][k];')
sub(sys.argv[1], F,
    'qk[k] = qk[k] + ((double)ws[1] * (double)r.ra) * gn[V - 1][k];',
    'qk[k] = qk[k] + ((double)ws[1] * (double)r.ra) * gn[0][k];')
