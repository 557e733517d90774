"""Second, independent restatement of the reference algorithm in pure-Python loops (small cases
only).  TEST INFRASTRUCTURE: it cross-checks oracle/vrt_oracle.c against transcription slips; it
is written line by line from the Julia source with 1-based indexing emulated by a leading dummy
element, and shares no code with the C oracle or the product.

Follows: src/voronoi_utils.jl:93-130,138-174 (_sort_by_layer_*), :186-245 (calc_Delaunay_lines),
:253-269 (reduce_layers), :360-396 (smallest_angle); src/functions.jl:392-395 (trapezoidal),
:484-500 (linear_weights); src/irregular_ray_tracing.jl:15-82,96-163 (Delaunay_upII/downII).
"""
import math
import struct


def sort_by_layer(neighbours, n_sites, boundary):
    """neighbours[i][j], 1-based i, j; neighbours[i][1] = count (voronoi_utils.jl:93-130)."""
    layers = [0] * (n_sites + 1)
    for i in range(1, n_sites + 1):
        n_nb = neighbours[i][1]
        for j in range(1, n_nb + 1):
            if neighbours[i][j + 1] == boundary:
                layers[i] = 1
    lower_layer = 1
    while True:
        for i in range(1, n_sites + 1):
            if layers[i] == 0:
                n_nb = neighbours[i][1]
                for j in range(1, n_nb + 1):
                    nb = neighbours[i][j + 1]
                    if nb > 0 and layers[nb] == lower_layer:
                        layers[i] = lower_layer + 1
                        break
        if not any(v == 0 for v in layers[1:]):
            break
        lower_layer += 1
    return layers


def sortperm(layers, n_sites):
    """Julia sortperm is stable; returns 1-based perm with a dummy at index 0."""
    return [0] + sorted(range(1, n_sites + 1), key=lambda i: layers[i])


def reduce_layers(sorted_layers):
    """sorted_layers: 1-based list (dummy at 0) -- voronoi_utils.jl:253-269."""
    n = len(sorted_layers) - 1
    reduced = [0] * (max(sorted_layers[1:]) + 2)
    reduced[1] = 1
    layer = 2
    for i in range(1, n + 1):
        if sorted_layers[i] == layer:
            reduced[layer] = i
            layer += 1
    reduced[len(reduced) - 1] = n
    return reduced


def _fdiv(a, b):
    """Float64 `/` as Julia evaluates it: x / 0.0 is +-Inf and 0.0 / 0.0 is NaN where Python raises."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)


def calc_delaunay_lines(positions, neighbours, n_sites, x_min, x_max, y_min, y_max):
    """positions[i] = [_, z, x, y] (1-based components) -- voronoi_utils.jl:186-245."""
    lines = {}
    for i in range(1, n_sites + 1):
        position = positions[i]
        x_r_r = x_max - position[2]
        x_r_l = position[2] - x_min
        y_r_r = y_max - position[3]
        y_r_l = position[3] - y_min
        n_nb = neighbours[i][1]
        for j in range(1, n_nb + 1):
            nb = neighbours[i][j + 1]
            if nb > 0:
                p_n = list(positions[nb])
                x_i_r = abs(x_max - p_n[2])
                x_i_l = abs(p_n[2] - x_min)
                if x_r_r + x_i_l < position[2] - p_n[2]:
                    p_n[2] = x_max + p_n[2] - x_min
                elif x_r_l + x_i_r < p_n[2] - position[2]:
                    p_n[2] = x_min + x_max - p_n[2]
                y_i_r = abs(y_max - p_n[3])
                y_i_l = abs(p_n[3] - y_min)
                if y_r_r + y_i_l < position[3] - p_n[3]:
                    p_n[3] = y_max + p_n[3] - y_min
                elif y_r_l + y_i_r < p_n[3] - position[3]:
                    p_n[3] = y_min + y_max - p_n[3]
                p_d = [0.0, p_n[1] - position[1], p_n[2] - position[2], p_n[3] - position[3]]
                nrm = math.sqrt((p_d[1] * p_d[1] + p_d[2] * p_d[2]) + p_d[3] * p_d[3])
                lines[(j, i)] = [0.0, _fdiv(p_d[1], nrm), _fdiv(p_d[2], nrm), _fdiv(p_d[3], nrm)]
    return lines


def smallest_angle(n, nbs, k, lines):
    """voronoi_utils.jl:360-396; nbs is the 1-based neighbour vector of site n."""
    dots = [0.0, -1.0, -1.0]
    indices = [0, None, None]
    for i in range(1, len(nbs)):
        nb = nbs[i]
        if nb > 0:
            norm_dir = lines[(i, n)]
            dot_product = (k[1] * norm_dir[1] + k[2] * norm_dir[2]) + k[3] * norm_dir[3]
            if dot_product > dots[2]:
                if dot_product > dots[1]:
                    dots[1] = dot_product
                    indices[1] = nb
                else:
                    dots[2] = dot_product
                    indices[2] = nb
    if dots[2] <= 0:
        dots[2] = 0.0
        indices[2] = indices[1]
    return dots, indices


def linear_weights(dtau):
    """functions.jl:484-500"""
    if dtau < 5e-4:
        e = 1 - dtau + 0.5 * dtau ** 2
        a = dtau * (1 / 2 - dtau / 3)
        b = dtau * (1 / 2 - dtau / 6)
    elif dtau > 50:
        e = 0.0
        a = 1 / dtau
        b = 1.0 - a
    else:
        e = math.exp(-dtau)
        a = (1 - e) / dtau - e
        b = 1 - a - e
    return a, b, e


def delaunay(up, k, S, I_0, alpha, positions, neighbours, lines, layers, perm, n_sweeps):
    """Delaunay_upII (up=True, irregular_ray_tracing.jl:15-82) / Delaunay_downII (:96-163).
    All sequences 1-based with a dummy first element; returns I likewise."""
    p = 7.0
    n = len(S) - 1
    I = [0.0] * (n + 1)
    max_layer = len(layers) - 1
    lower_idx = layers[2] - 1
    for t in range(1, lower_idx + 1):
        I[perm[t]] = I_0[t]
    for layer in range(2, max_layer):
        lower_idx = layers[layer]
        upper_idx = layers[layer + 1]
        for _sweep in range(1, n_sweeps + 1):
            order = range(lower_idx, upper_idx) if up else range(upper_idx - 1, lower_idx - 1, -1)
            for i in order:
                idx = perm[i]
                position = positions[idx]
                n_nb = neighbours[idx][1]
                nbs = [0] + [neighbours[idx][j] for j in range(2, n_nb + 2)]
                dots, upwind = smallest_angle(idx, nbs, k, lines)
                s = dots[1] ** p + dots[2] ** p
                w = [0.0, dots[1] ** p / s, dots[2] ** p / s]
                I[idx] = 0.0
                for rn in (1, 2):
                    u = upwind[rn]
                    up_pos = positions[u]
                    r = math.sqrt(((position[1] - up_pos[1]) ** 2 + (position[2] - up_pos[2]) ** 2)
                                  + (position[3] - up_pos[3]) ** 2)
                    dtau = r * (alpha[idx] + alpha[u]) / 2
                    a, b, e = linear_weights(dtau)
                    I[idx] += (e * I[u] + a * S[u] + b * S[idx]) * w[rn]
    return I


# ---- storage model of the product's fp32 storage path (second transcription of orc_delaunay_model) ----
# Written from the description in vrt_oracle.c, not from its code: the geometry of a site (upwind ids, weights,
# path lengths) is hoisted per layer, the sweeps run on those terms.  Every floating-point expression keeps the
# association of the reference's line (irregular_ray_tracing.jl:66-76, functions.jl:484-500), with squares
# written as products, so that the two transcriptions can be compared bit for bit.
def through_float(v):
    """double -> nearest float32 (ties to even, gradual underflow) -> double"""
    return struct.unpack("f", struct.pack("f", v))[0]


def linear_weights_eps(dtau, exp_eps=0.0):
    """linear_weights with every exp(-dtau) multiplied by (1 + exp_eps)"""
    if dtau < 5e-4:
        e = 1 - dtau + 0.5 * (dtau * dtau)
        a = dtau * (1 / 2 - dtau / 3)
        b = dtau * (1 / 2 - dtau / 6)
    elif dtau > 50:
        e = 0.0
        a = 1 / dtau
        b = 1.0 - a
    else:
        e = math.exp(-dtau) * (1.0 + exp_eps)
        a = (1 - e) / dtau - e
        b = 1 - a - e
    return a, b, e


def delaunay_model(up, k, S, I_0, alpha, positions, neighbours, lines, layers, perm, n_sweeps,
                   store="f64", coef="f64", exp_eps=0.0):
    """Delaunay_upII / Delaunay_downII with the intensities rounded to float32 never (store "f64"), when a
    layer's last sweep is done ("layer") or at every site update ("visit"); coef "f32": the constant term and
    the two in-layer couplings of a site are formed once per layer, rounded to float32, and reused by the
    sweeps.  All sequences 1-based with a dummy first element, as in delaunay()."""
    p = 7.0
    n = len(S) - 1
    I = [0.0] * (n + 1)
    rank = [0] * (n + 1)
    for t in range(1, n + 1):
        rank[perm[t]] = t
    for t in range(1, layers[2]):
        I[perm[t]] = I_0[t]                      # the boundary layer takes I_0 as given
    for layer in range(2, len(layers) - 1):
        lo, hi = layers[layer], layers[layer + 1]
        terms = {}
        for i in range(lo, hi):
            idx = perm[i]
            n_nb = neighbours[idx][1]
            nbs = [0] + [neighbours[idx][j] for j in range(2, n_nb + 2)]
            dots, upwind = smallest_angle(idx, nbs, k, lines)
            s = dots[1] ** p + dots[2] ** p
            site = []
            for rn in (1, 2):
                u = upwind[rn]
                dz = positions[idx][1] - positions[u][1]
                dx = positions[idx][2] - positions[u][2]
                dy = positions[idx][3] - positions[u][3]
                r = math.sqrt((dz * dz + dx * dx) + dy * dy)
                a, b, e = linear_weights_eps(r * (alpha[idx] + alpha[u]) / 2, exp_eps)
                site.append((u, dots[rn] ** p / s, a, b, e))
            terms[idx] = site
        kept = {}
        if coef == "f32":
            for idx, site in terms.items():
                t, g = [], []
                for u, w, a, b, e in site:
                    if rank[u] < lo:             # earlier layer: its intensity is final
                        t.append((e * I[u] + a * S[u] + b * S[idx]) * w)
                    else:
                        t.append((a * S[u] + b * S[idx]) * w)
                    g.append(through_float(e * w if lo <= rank[u] < hi else 0.0))
                kept[idx] = (through_float(t[0] + t[1]), g[0], g[1])
        for _sweep in range(n_sweeps):
            for i in (range(lo, hi) if up else range(hi - 1, lo - 1, -1)):
                idx = perm[i]
                site = terms[idx]
                if coef == "f32":
                    c, g1, g2 = kept[idx]
                    v = c + g1 * I[site[0][0]] + g2 * I[site[1][0]]
                else:
                    v = 0.0
                    for u, w, a, b, e in site:
                        v += (e * I[u] + a * S[u] + b * S[idx]) * w
                I[idx] = through_float(v) if store == "visit" else v
        if store == "layer":
            for i in range(lo, hi):
                I[perm[i]] = through_float(I[perm[i]])
    return I
