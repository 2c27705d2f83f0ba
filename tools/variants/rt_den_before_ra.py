"""k_render_plane mutant (profiles/render_rt/mutants.txt): den accumulated before the test of ra, and ra dropped from wr
(the same for a live ray, whose ra is 1; a dead ray now counts in den)."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '            if (!(r.ra != 0.0f)) continue;\n',
    '            for (int side = 0; side < V; ++side) den[side] += (double)w[side];\n            if (!(r.ra != 0.0f)) continue;\n')
sub(sys.argv[1], F,
    '                wr[side] = (double)w[side] * (double)r.ra;\n                den[side] += wr[side];\n',
    '                wr[side] = (double)w[side];\n')
