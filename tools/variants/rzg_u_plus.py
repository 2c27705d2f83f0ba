"""k_render_layers_depth_grad mutant (profiles/render_depth_grad/mutants.txt): u taken to grow with px, as v does with
py (u = Wt/2 - px inv in the forward): both terms add Pu's part."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F, '(Pv * sy - Pu * sx)', '(Pv * sy + Pu * sx)', count=2)
sub(sys.argv[1], F, 'Pv * (double)there.oy - Pu * (double)there.ox', 'Pv * (double)there.oy + Pu * (double)there.ox', count=2)
