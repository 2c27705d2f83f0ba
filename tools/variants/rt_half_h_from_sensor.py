"""k_render_plane mutant (profiles/render_rt/mutants.txt): half_h from the SENSOR's height -- right whenever Ht == H."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    'half_h = (float)a.Ht * 0.5f',
    'half_h = (float)a.H * 0.5f')
