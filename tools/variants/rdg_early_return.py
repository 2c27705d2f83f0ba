"""k_render_layers_dp_grad mutant (profiles/render_dp_grad/mutants.txt): lanes past H W return before the reduction instead of taking part in
it with zeros: the last wave's shuffles read lanes that are no longer there."""
import sys

from _edit import sub

F = "sdirt_render_rt.hip"
sub(sys.argv[1], F,
    '    double acc[3] = {};\n    if (p < HW) {\n        const int i = (int)(p / e.W), j = (int)(p - (int64_t)i * e.W);\n        const float ox = e.x1[j], oy = e.y1[i];',
    '    double acc[3] = {};\n    if (p >= HW) return;\n    if (p < HW) {\n        const int i = (int)(p / e.W), j = (int)(p - (int64_t)i * e.W);\n        const float ox = e.x1[j], oy = e.y1[i];')
