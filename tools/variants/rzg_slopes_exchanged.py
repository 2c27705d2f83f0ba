"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): the ray's two slopes exchanged in gz,
Pv sx - Pu sy, with and without a coverage."""
import sys

from _edit import sub

sub(sys.argv[1], "sdirt_render_rt.hip", '(Pv * sy - Pu * sx)', '(Pv * sx - Pu * sy)', count=2)
