"""k_render_plane mutant (profiles/render_rt/mutants.txt): half_w computed from the texture's HEIGHT."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'half_w = (float)a.Wt * 0.5f',
    'half_w = (float)a.Ht * 0.5f')
