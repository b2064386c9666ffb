// host_model.cpp -- OBJ/MTL reader, CreateGeometry tables and the KD-tree build.
//
// Reader semantics: CVMCTracer/CVMCTracer/Framework/ObjReader.cpp:8-259 and
// ObjReader.hpp:37-139 (dummy index 0, map-ordered groups, fan triangulation,
// "Ks" implies Ns=2, newmtl re-uses an existing name).  Numbers are parsed
// with strtof/strtod, which is what std::istream >> float/double resolves to.
//
// KD build semantics: MCRT/QuinEngine/Utils/KDTree.hpp:58-287 -- see
// build_kdtree() below; the BFS flatten follows RTX/ShaderResource.hpp:128-179.
#include "host_model.hpp"

#include <algorithm>
#include <array>
#include <cmath>
#include <cctype>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <fstream>
#include <map>
#include <numeric>
#include <sstream>

#include "../../include/mcpt.h"

namespace mcpt {
namespace {

// ---- whitespace tokenizer with istream-like extraction ---------------------
struct Cursor {
    const char* p;
    const char* end;
    bool fail = false;

    void skip() {
        while (p < end && std::isspace(static_cast<unsigned char>(*p))) ++p;
    }
    bool token(std::string& out) {          // operator>>(std::string&)
        if (fail) return false;
        skip();
        if (p >= end) { fail = true; return false; }
        const char* b = p;
        while (p < end && !std::isspace(static_cast<unsigned char>(*p))) ++p;
        out.assign(b, p);
        return true;
    }
    // operator>>(float&) / (double&): value 0 on failure
    template <typename T>
    T number() {
        if (fail) return T(0);
        skip();
        std::string tmp(p, std::min<size_t>(static_cast<size_t>(end - p), 128));
        char* e = nullptr;
        T v;
        if constexpr (std::is_same<T, float>::value) v = std::strtof(tmp.c_str(), &e);
        else v = std::strtod(tmp.c_str(), &e);
        if (e == tmp.c_str()) { fail = true; return T(0); }
        p += (e - tmp.c_str());
        return v;
    }
};

// ObjReader.hpp:90-138 ("v", "v/t", "v//n", "v/t/n")
bool parse_face_vertex(const std::string& tok, int32_t& v, int32_t& t, int32_t& n) {
    const char* s = tok.c_str();
    auto get_int = [&](int32_t& out) -> bool {
        const char* q = s;
        if (*q == '+' || *q == '-') ++q;
        if (!std::isdigit(static_cast<unsigned char>(*q))) { out = 0; return false; }
        char* e = nullptr;
        out = static_cast<int32_t>(std::strtol(s, &e, 10));
        s = e;
        return true;
    };
    auto get_char = [&]() -> bool {
        while (*s && std::isspace(static_cast<unsigned char>(*s))) ++s;
        if (!*s) return false;
        ++s;
        return true;
    };
    if (!get_int(v)) return false;
    if (!get_char()) { t = 0; n = 0; return true; }
    if (!get_int(t)) {
        t = 0;
        get_char();
        return get_int(n);
    }
    if (!get_char()) { n = 0; return true; }
    return get_int(n);
}

std::string slurp(const std::string& path) {
    std::ifstream f(path, std::ios::binary);
    if (!f.is_open()) throw Error{MCPT_E_IO, "Can't open file " + path};
    std::ostringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

// std::getline with trailing-backslash continuation (ObjReader.cpp:23-34)
template <typename F>
void for_each_line(const std::string& text, F&& fn) {
    size_t pos = 0;
    std::string line;
    while (pos < text.size()) {
        line.clear();
        for (;;) {
            size_t e = text.find('\n', pos);
            size_t len = (e == std::string::npos ? text.size() : e) - pos;
            line.append(text, pos, len);
            pos = (e == std::string::npos) ? text.size() : e + 1;
            if (!line.empty() && line.back() == '\\' && pos < text.size()) {
                line.pop_back();
                continue;
            }
            break;
        }
        fn(line);
    }
}

int find_material(const ObjModel& m, const std::string& name) {   // ObjReader.hpp:78-88
    for (size_t i = 1; i < m.materials.size(); ++i)
        if (m.materials[i].name == name) return static_cast<int>(i);
    return 0;
}

void read_mtl(ObjModel& m, const std::string& path) {   // ObjReader.cpp:163-259
    const std::string text = slurp(path);
    int idx = 0;
    std::string tok;
    for_each_line(text, [&](const std::string& line) {
        Cursor c{line.data(), line.data() + line.size()};
        if (!c.token(tok) || tok[0] == '#') return;
        if (tok == "newmtl") {
            c.token(tok);
            idx = find_material(m, tok);
            if (idx == 0) {
                ObjMaterial mt;
                mt.name = tok;
                m.materials.push_back(mt);
                idx = static_cast<int>(m.materials.size()) - 1;
            }
        } else if (tok == "Ka" || tok == "Kd" || tok == "Ks") {
            Vec3 v;
            v.x = c.number<float>();
            v.y = c.number<float>();
            v.z = c.number<float>();
            ObjMaterial& mt = m.materials[idx];
            if (tok[1] == 'a') mt.Ka = v;
            else if (tok[1] == 'd') mt.Kd = v;
            else { mt.Ks = v; mt.Ns = 2; }
        } else if (tok == "Ns") {
            m.materials[idx].Ns = c.number<double>();
        } else if (tok == "Tr") {
            m.materials[idx].Tr = c.number<double>();
        } else if (tok == "Ni") {
            m.materials[idx].Ni = c.number<double>();
        }
    });
}

// tinyobjloader v1.1.1's MTL semantics (QE/3rdparty/include/tiny_obj_loader.h
// LoadMtl, the loader QuinEngine uses, QE/Utils/Structure.hpp:9-12): every
// newmtl appends (a lookup finds the first of a name), InitMaterial defaults
// (Ka Kd Ks 0, shininess 1, ior 1, dissolve 1), Ks does not touch Ns, `d`
// sets dissolve and wins over `Tr`, which sets dissolve = 1 - Tr; QuinEngine
// then uploads Tr = 1 - dissolve (RTX/ShaderResource.hpp:204-215), in float.
void read_mtl_tinyobj(ObjModel& m, const std::string& path) {
    const std::string text = slurp(path);
    int idx = -1;
    bool has_d = false, has_tr = false;
    float dissolve = 1.0f;
    std::string tok;
    auto flush = [&]() {
        if (idx >= 0) m.materials[static_cast<size_t>(idx)].Tr = static_cast<double>(1.0f - dissolve);
    };
    for_each_line(text, [&](const std::string& line) {
        Cursor c{line.data(), line.data() + line.size()};
        if (!c.token(tok) || tok[0] == '#') return;
        if (tok == "newmtl") {
            flush();
            c.token(tok);
            ObjMaterial mt;
            mt.name = tok;
            mt.Ns = 1.0;
            mt.Ni = 1.0;
            m.materials.push_back(mt);
            idx = static_cast<int>(m.materials.size()) - 1;
            has_d = has_tr = false;
            dissolve = 1.0f;
            return;
        }
        if (idx < 0) return;
        ObjMaterial& mt = m.materials[static_cast<size_t>(idx)];
        if (tok == "Ka" || tok == "Kd" || tok == "Ks") {
            Vec3 v;
            v.x = static_cast<float>(c.number<double>());
            v.y = static_cast<float>(c.number<double>());
            v.z = static_cast<float>(c.number<double>());
            (tok[1] == 'a' ? mt.Ka : (tok[1] == 'd' ? mt.Kd : mt.Ks)) = v;
        } else if (tok == "Ns") {
            mt.Ns = static_cast<float>(c.number<double>());
        } else if (tok == "Ni") {
            mt.Ni = static_cast<float>(c.number<double>());
        } else if (tok == "d") {
            dissolve = static_cast<float>(c.number<double>());
            has_d = true;
        } else if (tok == "Tr") {
            if (!has_d) dissolve = 1.0f - static_cast<float>(c.number<double>());
            has_tr = true;
        }
    });
    flush();
    (void)has_tr;
}

int find_material_tinyobj(const ObjModel& m, const std::string& name) {   // material_map: the first of a name
    for (size_t i = 1; i < m.materials.size(); ++i)
        if (m.materials[i].name == name) return static_cast<int>(i);
    return 0;                                                                // -1 in tinyobj: the zero material
}

// tinyobjloader's OBJ semantics (LoadObj, tiny_obj_loader.h:1712-2000), as
// QuinEngine consumes them (RTX/ShaderResource.hpp:88-104: shapes in file
// order, a material id per triangle): every `g` / `o` line starts a shape
// (named by the first name after `g`, the rest of the line after `o`; the
// first shape is unnamed), `usemtl` switches the per-face material without
// ending the shape, faces are fan-triangulated (v0, v[k-1], v[k]).  In the
// ObjModel a group is a run of one shape's faces with one material, keyed
// "%06d:<shape name>" so the std::map order -- CreateGeometry's order and the
// brute-force rank -- is the file order, and each geometry's material is its
// faces' own.  The dummy material 0 (tinyobj's id -1) is all zero, as an
// out-of-range StructuredBuffer read returns.
void read_obj_tinyobj(const std::string& path, ObjModel& m) {
    m = ObjModel();
    m.path = path;
    m.vertices.push_back(Vec3{});
    m.n_texcoords = 1;
    m.normals.push_back(Vec3{});
    m.triangles.push_back(ObjTriangle{});
    ObjMaterial zero;
    zero.Ns = 0.0;
    zero.Ni = 0.0;
    m.materials.push_back(zero);
    const std::string text = slurp(path);
    std::string shape_name;
    int material = 0, run_material = -1, runs = 0;
    std::vector<int32_t>* group = nullptr;
    bool new_shape = true;
    std::string tok;
    auto face_group = [&]() -> std::vector<int32_t>* {
        if (new_shape || material != run_material) {
            char key[32];
            std::snprintf(key, sizeof key, "%06d:", runs++);
            group = &m.groups[key + shape_name];
            run_material = material;
            new_shape = false;
        }
        return group;
    };
    for_each_line(text, [&](const std::string& line) {
        Cursor c{line.data(), line.data() + line.size()};
        if (!c.token(tok) || tok[0] == '#') return;
        if (tok == "v" || tok == "vn") {
            Vec3 v;
            v.x = static_cast<float>(c.number<double>());
            v.y = static_cast<float>(c.number<double>());
            v.z = static_cast<float>(c.number<double>());
            (tok.size() == 1 ? m.vertices : m.normals).push_back(v);
        } else if (tok == "vt") {
            ++m.n_texcoords;
        } else if (tok == "f") {
            std::vector<int32_t>* g = face_group();
            std::vector<std::array<int32_t, 3>> fv;
            std::string vt;
            while (c.token(vt)) {
                int32_t vi, ti, ni;
                if (!parse_face_vertex(vt, vi, ti, ni)) throw Error{MCPT_E_PARSE, "Invalid OBJ file!"};
                // negative indices count back from the end (tinyobj fixIndex)
                if (vi < 0) vi += static_cast<int32_t>(m.vertices.size());
                if (ti < 0) ti += static_cast<int32_t>(m.n_texcoords);
                if (ni < 0) ni += static_cast<int32_t>(m.normals.size());
                fv.push_back({vi, ti, ni});
            }
            for (size_t k = 2; k < fv.size(); ++k) {
                ObjTriangle t;
                t.material = material;
                const std::array<int32_t, 3>* q[3] = {&fv[0], &fv[k - 1], &fv[k]};
                for (int j = 0; j < 3; ++j) { t.v[j] = (*q[j])[0]; t.t[j] = (*q[j])[1]; t.n[j] = (*q[j])[2]; }
                m.triangles.push_back(t);
                g->push_back(static_cast<int32_t>(m.triangles.size() - 1));
            }
        } else if (tok == "g") {
            shape_name = c.token(tok) ? tok : std::string();
            new_shape = true;
        } else if (tok == "o") {
            c.skip();
            shape_name.assign(c.p, c.end);
            while (!shape_name.empty() && std::isspace(static_cast<unsigned char>(shape_name.back())))
                shape_name.pop_back();
            new_shape = true;
        } else if (tok == "usemtl") {
            c.token(tok);
            material = find_material_tinyobj(m, tok);
        } else if (tok == "mtllib") {
            c.token(tok);
            size_t slash = path.find_last_of('/');
            std::string dir = (slash == std::string::npos) ? std::string(".") : path.substr(0, slash);
            read_mtl_tinyobj(m, dir + "/" + tok);
        }
    });
}

}  // namespace

void read_obj(const std::string& path, ObjModel& m, int flavor) {
    if (flavor == MCPT_OBJ_TINYOBJ) {
        read_obj_tinyobj(path, m);
        return;
    }
    read_obj_cv(path, m);
}

void read_obj_cv(const std::string& path, ObjModel& m) {   // ObjReader.cpp:8-161
    m = ObjModel();
    m.path = path;
    m.vertices.push_back(Vec3{});
    m.n_texcoords = 1;
    m.normals.push_back(Vec3{});
    m.triangles.push_back(ObjTriangle{});
    m.materials.push_back(ObjMaterial{});
    const std::string text = slurp(path);
    std::vector<int32_t>* group = &m.groups["default"];
    int material = 0;
    std::string tok;
    for_each_line(text, [&](const std::string& line) {
        Cursor c{line.data(), line.data() + line.size()};
        if (!c.token(tok) || tok[0] == '#') return;
        if (tok == "v" || tok == "vn") {
            Vec3 v;
            v.x = c.number<float>();
            v.y = c.number<float>();
            v.z = c.number<float>();
            (tok.size() == 1 ? m.vertices : m.normals).push_back(v);
        } else if (tok == "f") {
            int k = 0;
            m.triangles.push_back(ObjTriangle{});
            m.triangles.back().material = material;
            group->push_back(static_cast<int32_t>(m.triangles.size() - 1));
            std::string vt;
            while (c.token(vt)) {
                int32_t vi, ti, ni;
                if (!parse_face_vertex(vt, vi, ti, ni)) throw Error{MCPT_E_PARSE, "Invalid OBJ file!"};
                if (k < 3) {
                    ObjTriangle& t = m.triangles.back();
                    t.v[k] = vi; t.t[k] = ti; t.n[k] = ni;
                } else {   // fan: (v0, previous v2, new)
                    ObjTriangle nt;
                    const ObjTriangle prev = m.triangles.back();
                    nt.material = material;
                    nt.v[0] = prev.v[0]; nt.v[1] = prev.v[2]; nt.v[2] = vi;
                    nt.t[0] = prev.t[0]; nt.t[1] = prev.t[2]; nt.t[2] = ti;
                    nt.n[0] = prev.n[0]; nt.n[1] = prev.n[2]; nt.n[2] = ni;
                    m.triangles.push_back(nt);
                    group->push_back(static_cast<int32_t>(m.triangles.size() - 1));
                }
                ++k;
            }
        } else if (tok == "vt") {
            ++m.n_texcoords;
        } else if (tok == "g") {
            c.token(tok);   // on failure tok keeps "g"
            group = &m.groups[tok];
        } else if (tok == "usemtl") {
            c.token(tok);
            material = find_material(m, tok);
        } else if (tok == "mtllib") {
            c.token(tok);
            size_t slash = path.find_last_of('/');
            std::string dir = (slash == std::string::npos) ? std::string(".") : path.substr(0, slash);
            read_mtl(m, dir + "/" + tok);
        }
    });
}

// ---------------------------------------------------------------------------
void build_host_scene(const ObjModel& m, HostScene& hs, const char* kd_cache_dir, int* cache_hit, int kd_build) {
    hs = HostScene();
    const int64_t ntri = static_cast<int64_t>(m.triangles.size());
    // CreateGeometry (CUTracer.cu:277-311): one record per non-empty group,
    // start = first triangle index, material of that triangle.
    for (const auto& kv : m.groups) {
        const auto& ids = kv.second;
        if (ids.empty()) continue;
        const ObjMaterial& mt = m.materials[static_cast<size_t>(m.triangles[static_cast<size_t>(ids[0])].material)];
        Geometry g;
        g.Ka = mt.Ka; g.Kd = mt.Kd; g.Ks = mt.Ks;
        g.Ns = static_cast<float>(mt.Ns);
        g.Tr = static_cast<float>(mt.Tr);
        g.Ni = static_cast<float>(mt.Ni);
        g.start = static_cast<uint32_t>(ids[0]);
        g.count = static_cast<uint32_t>(ids.size());
        hs.geoms.push_back(g);
    }
    // the brute-force loop (CUTracer.cu:49-54) tests triangle start+i of each
    // geometry in order: rank = position in that loop, geometry = first cover
    std::vector<int32_t> geom_of(static_cast<size_t>(ntri), -1);
    std::vector<uint32_t> rank_of(static_cast<size_t>(ntri), 0);
    uint32_t rank = 0;
    for (size_t g = 0; g < hs.geoms.size(); ++g) {
        for (uint32_t i = 0; i < hs.geoms[g].count; ++i, ++rank) {
            uint64_t cv = static_cast<uint64_t>(hs.geoms[g].start) + i;
            if (cv >= static_cast<uint64_t>(ntri))
                throw Error{MCPT_E_INVALID, "geometry range exceeds the triangle count"};
            if (geom_of[cv] < 0) {
                geom_of[cv] = static_cast<int32_t>(g);
                rank_of[cv] = rank;
            }
        }
    }
    const int64_t nv = static_cast<int64_t>(m.vertices.size());
    const int64_t nn = static_cast<int64_t>(m.normals.size());
    for (int64_t i = 0; i < ntri; ++i) {
        if (geom_of[static_cast<size_t>(i)] < 0) continue;
        const ObjTriangle& t = m.triangles[static_cast<size_t>(i)];
        for (int j = 0; j < 3; ++j) {
            if (t.v[j] < 0 || t.v[j] >= nv || t.n[j] < 0 || t.n[j] >= nn)
                throw Error{MCPT_E_INVALID, "triangle " + std::to_string(i) + " has an out-of-range index"};
            // a non-finite vertex makes every KD box it touches inf/NaN (the
            // reference renders garbage there); refuse it
            const Vec3& p = m.vertices[static_cast<size_t>(t.v[j])];
            if (!std::isfinite(p.x) || !std::isfinite(p.y) || !std::isfinite(p.z))
                throw Error{MCPT_E_INVALID, "triangle " + std::to_string(i) + " has a non-finite vertex"};
        }
        hs.kd_tris.push_back(static_cast<int32_t>(i));
        hs.kd_geom.push_back(static_cast<uint32_t>(geom_of[static_cast<size_t>(i)]));
        hs.kd_prio.push_back(rank_of[static_cast<size_t>(i)]);
        for (int j = 0; j < 3; ++j) {
            const Vec3& p = m.vertices[static_cast<size_t>(t.v[j])];
            const Vec3& q = m.normals[static_cast<size_t>(t.n[j])];
            hs.kd_verts.insert(hs.kd_verts.end(), {p.x, p.y, p.z});
            hs.kd_normals.insert(hs.kd_normals.end(), {q.x, q.y, q.z});
        }
    }
    if (cache_hit) *cache_hit = 0;
    hs.kd_build = kd_build;
    if (kd_cache_dir && *kd_cache_dir) {
        if (kd_cache_load(kd_cache_dir, hs.kd_verts, hs.nodes, hs.leaf_ids, hs.kd_depth, kd_build)) {
            if (cache_hit) *cache_hit = 1;
            return;
        }
        build_kdtree(hs.kd_verts, hs.nodes, hs.leaf_ids, hs.kd_depth, kd_build);
        kd_cache_store(kd_cache_dir, hs.kd_verts, hs.nodes, hs.leaf_ids, hs.kd_depth, kd_build);   // best effort
        return;
    }
    build_kdtree(hs.kd_verts, hs.nodes, hs.leaf_ids, hs.kd_depth, kd_build);
}

// ---------------------------------------------------------------------------
// Terminal cull: may the path loop's last query (CUTracer.cu:162-175, which
// adds color * Ka(hit) * illum) be skipped for a ray that can reach no emitter?
// Yes when only emitters (any Ka component > 0, CUTracer.cu:111) have a Ka
// other than zero -- a negative or NaN Ka on any other geometry is radiance the
// query must collect -- and every Kd and Ks is finite, so the throughput the
// zero multiplies comes from finite factors.  Then one AABB per emitter
// geometry over its triangles' vertices (all finite, build_host_scene).
int terminal_cull_boxes(const HostScene& hs, float (*boxes)[6], int max_boxes) {
    auto finite3 = [](const Vec3& v) { return std::isfinite(v.x) && std::isfinite(v.y) && std::isfinite(v.z); };
    std::vector<int> box_of(hs.geoms.size(), -1);
    int n = 0;
    for (size_t g = 0; g < hs.geoms.size(); ++g) {
        const Geometry& ge = hs.geoms[g];
        if (!finite3(ge.Kd) || !finite3(ge.Ks)) return 0;
        if (ge.Ka.x > 0 || ge.Ka.y > 0 || ge.Ka.z > 0) {
            if (n == max_boxes) return 0;          // (boxes are not merged)
            for (int a = 0; a < 3; ++a) {
                boxes[n][a] = INFINITY;            // empty until a triangle widens it: always culled
                boxes[n][3 + a] = -INFINITY;
            }
            box_of[g] = n++;
        } else if (!(ge.Ka.x == 0 && ge.Ka.y == 0 && ge.Ka.z == 0)) {
            return 0;
        }
    }
    for (size_t k = 0; k < hs.kd_geom.size(); ++k) {
        const int b = box_of[hs.kd_geom[k]];
        if (b < 0) continue;
        const float* v = &hs.kd_verts[9 * k];
        for (int j = 0; j < 3; ++j)
            for (int a = 0; a < 3; ++a) {
                boxes[b][a] = std::min(boxes[b][a], v[3 * j + a]);
                boxes[b][3 + a] = std::max(boxes[b][3 + a], v[3 * j + a]);
            }
    }
    return n;
}

// ---------------------------------------------------------------------------
// Light table: the emitters' triangles as the direct-lighting queries sample them,
// uniformly by area (host_model.hpp).  Every product and sum below is one double
// operation (the build contracts nothing), so a restatement in double reproduces
// the table bit for bit.
void light_table(const HostScene& hs, LightTable& out) {
    out = LightTable{};
    std::vector<double> running;
    double S = 0.0;
    for (size_t k = 0; k < hs.kd_geom.size(); ++k) {
        const Geometry& ge = hs.geoms[hs.kd_geom[k]];
        if (!(ge.Ka.x > 0 || ge.Ka.y > 0 || ge.Ka.z > 0)) continue;
        const float* v = &hs.kd_verts[9 * k];
        double e1[3], e2[3];
        for (int a = 0; a < 3; ++a) {
            e1[a] = double(v[3 + a]) - double(v[a]);
            e2[a] = double(v[6 + a]) - double(v[a]);
        }
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2],
                             e1[0] * e2[1] - e1[1] * e2[0]};
        const double len = std::sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
        const double area = 0.5 * len;
        if (!(area > 0.0)) continue;
        S = S + area;
        running.push_back(S);
        out.kd_ids.push_back(static_cast<int32_t>(k));
        for (int a = 0; a < 3; ++a) out.normals.push_back(static_cast<float>(c[a] / len));
    }
    out.cdf.reserve(running.size());
    for (double s : running) out.cdf.push_back(static_cast<float>(s / S));
    out.area_total = static_cast<float>(S);
}

// ---------------------------------------------------------------------------
// Miss cull: occluder boxes.  A secondary ray whose segment misses the box of
// every triangle has no hit, so the shade that creates it may end the path at
// once (trace_device.hpp scene_box_hits).  The boxes need no material
// knowledge: bottom-up clustering from one box per triangle, always merging
// the pair whose union adds the least volume (then the least surface area,
// then the lower indices: deterministic), until max_boxes or fewer are left
// and no merge is free.  Coplanar wall triangles merge at zero cost and stay
// flat; a mesh ends as one box or a few.
// Cost: every box keeps its cheapest partner, so a merge rescans only the
// boxes that pointed at the merged pair -- O(n^2) pair costs up front, O(n)
// per merge after that.  Above kMissCullExact triangles (C4's 70k mesh) the
// triangles are pre-bucketed first: an axis-flat triangle by its plane (axis,
// coordinate), any other by the cell of its centroid in an 8^3 grid over the
// scene bounds, one box per bucket; should the planes alone exceed the limit
// (a voxel mesh), flat triangles go to the grid too.
namespace {

constexpr size_t kMissCullExact = 2048;

struct CBox {
    float lo[3], hi[3];
    void add(const CBox& b) {
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], b.lo[a]); hi[a] = std::max(hi[a], b.hi[a]); }
    }
    double vol() const {
        return (double(hi[0]) - lo[0]) * (double(hi[1]) - lo[1]) * (double(hi[2]) - lo[2]);
    }
    double area() const {
        const double x = double(hi[0]) - lo[0], y = double(hi[1]) - lo[1], z = double(hi[2]) - lo[2];
        return x * y + y * z + z * x;
    }
};

struct PairCost {
    double dv, da;
    size_t j;
    bool operator<(const PairCost& o) const {
        if (dv != o.dv) return dv < o.dv;
        if (da != o.da) return da < o.da;
        return j < o.j;
    }
    bool free() const { return dv <= 0.0 && da <= 0.0; }
};

PairCost pair_cost(const std::vector<CBox>& bx, size_t i, size_t j) {
    CBox u = bx[i];
    u.add(bx[j]);
    return {u.vol() - bx[i].vol() - bx[j].vol(), u.area() - bx[i].area() - bx[j].area(), j};
}

void cluster_boxes(std::vector<CBox>& bx, size_t max_boxes) {
    const size_t n = bx.size();
    const PairCost none{INFINITY, INFINITY, n};
    std::vector<char> live(n, 1);
    std::vector<PairCost> best(n, none);
    auto rescan = [&](size_t i) {
        best[i] = none;
        for (size_t j = 0; j < n; ++j)
            if (j != i && live[j]) best[i] = std::min(best[i], pair_cost(bx, i, j));
    };
    for (size_t i = 0; i < n; ++i) rescan(i);
    for (size_t alive = n; alive > 1; --alive) {
        size_t i = n;
        for (size_t k = 0; k < n; ++k)
            if (live[k] && (i == n || best[k] < best[i])) i = k;
        if (alive <= max_boxes && !best[i].free()) break;
        size_t j = best[i].j;
        if (j < i) std::swap(i, j);                    // the union stays in the lower slot
        bx[i].add(bx[j]);
        live[j] = 0;
        rescan(i);
        for (size_t k = 0; k < n; ++k) {
            if (!live[k] || k == i) continue;
            if (best[k].j == i || best[k].j == j) rescan(k);
            else best[k] = std::min(best[k], pair_cost(bx, k, i));
        }
    }
    size_t m = 0;
    for (size_t k = 0; k < n; ++k)
        if (live[k]) bx[m++] = bx[k];
    bx.resize(m);
}

}  // namespace

int miss_cull_boxes(const HostScene& hs, float (*boxes)[6], int max_boxes) {
    const size_t nt = hs.kd_verts.size() / 9;
    if (!nt || max_boxes < 1) return 0;
    for (float v : hs.kd_verts)
        if (!std::isfinite(v)) return 0;
    std::vector<CBox> tb(nt);
    CBox all{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
    for (size_t k = 0; k < nt; ++k) {
        const float* v = &hs.kd_verts[9 * k];
        CBox b{{v[0], v[1], v[2]}, {v[0], v[1], v[2]}};
        for (int j = 1; j < 3; ++j) b.add(CBox{{v[3 * j], v[3 * j + 1], v[3 * j + 2]}, {v[3 * j], v[3 * j + 1], v[3 * j + 2]}});
        tb[k] = b;
        all.add(b);
    }
    std::vector<CBox> bx;
    if (nt <= kMissCullExact) {
        bx = tb;
    } else {
        // buckets in key order (std::map): planes first, then grid cells
        for (int with_planes = 1; with_planes >= 0; --with_planes) {
            std::map<std::pair<int, uint32_t>, CBox> buckets;
            for (const CBox& b : tb) {
                std::pair<int, uint32_t> key{3, 0u};
                for (int a = 0; a < 3 && with_planes; ++a)
                    if (b.lo[a] == b.hi[a] && key.first == 3) {
                        const float c = b.lo[a] + 0.0f;            // (-0 and +0: one plane)
                        uint32_t bits;
                        std::memcpy(&bits, &c, 4);
                        key = {a, bits};
                    }
                if (key.first == 3) {
                    for (int a = 0; a < 3; ++a) {
                        const double ext = double(all.hi[a]) - all.lo[a];
                        const double c = (double(b.lo[a]) + b.hi[a]) * 0.5 - all.lo[a];
                        const int cell = ext > 0.0 ? std::min(7, std::max(0, int(c / ext * 8.0))) : 0;
                        key.second = key.second * 8u + uint32_t(cell);
                    }
                }
                auto it = buckets.find(key);
                if (it == buckets.end()) buckets.emplace(key, b);
                else it->second.add(b);
            }
            bx.clear();
            for (const auto& kv : buckets) bx.push_back(kv.second);
            if (bx.size() <= kMissCullExact) break;
        }
    }
    // the free merges first: they leave every wall as one flat box, which is
    // what tells a closed room (the test could only cost there)
    cluster_boxes(bx, bx.size());
    bool face[3][2] = {};
    for (const CBox& b : bx) {
        for (int a = 0; a < 3; ++a) {
            if (b.lo[a] != b.hi[a]) continue;
            bool covers = true;
            for (int c = 0; c < 3; ++c)
                if (c != a) covers = covers && b.lo[c] <= all.lo[c] && b.hi[c] >= all.hi[c];
            if (covers && b.lo[a] == all.lo[a]) face[a][0] = true;
            if (covers && b.lo[a] == all.hi[a]) face[a][1] = true;
        }
    }
    if (face[0][0] && face[0][1] && face[1][0] && face[1][1] && face[2][0] && face[2][1]) return 0;
    cluster_boxes(bx, static_cast<size_t>(max_boxes));
    for (const CBox& b : bx) {   // a box over the whole scene: every ray that can hit anything passes
        bool spans = true;
        for (int a = 0; a < 3; ++a) spans = spans && b.lo[a] <= all.lo[a] && b.hi[a] >= all.hi[a];
        if (spans) return 0;
    }
    for (size_t k = 0; k < bx.size(); ++k)
        for (int a = 0; a < 3; ++a) {
            boxes[k][a] = bx[k].lo[a];
            boxes[k][3 + a] = bx[k].hi[a];
        }
    return static_cast<int>(bx.size());
}

void direct_list_assign(const HostScene& hs, const float (*boxes)[6], int n_boxes, std::vector<int32_t>& tri_box) {
    const size_t nt = hs.kd_verts.size() / 9;
    tri_box.assign(nt, -1);
    for (size_t k = 0; k < nt; ++k) {
        const float* v = &hs.kd_verts[9 * k];
        for (int b = 0; b < n_boxes && tri_box[k] < 0; ++b) {
            bool in = true;
            for (int j = 0; j < 3; ++j)
                for (int a = 0; a < 3; ++a) in = in && v[3 * j + a] >= boxes[b][a] && v[3 * j + a] <= boxes[b][3 + a];
            if (in) tri_box[k] = b;
        }
    }
}

uint32_t clip_spheres(const HostScene& hs, const float (*boxes)[6], int n_boxes, const std::vector<int32_t>& tri_box,
                      uint32_t want, double margin, double max_reach, float (*spheres)[4]) {
    const size_t nt = hs.kd_verts.size() / 9;
    double smin[3] = {INFINITY, INFINITY, INFINITY}, smax[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (size_t k = 0; k < nt; ++k)
        for (int j = 0; j < 9; ++j) {
            const double v = hs.kd_verts[9 * k + j];
            smin[j % 3] = std::min(smin[j % 3], v);
            smax[j % 3] = std::max(smax[j % 3], v);
        }
    double diag2 = 0.0;
    for (int a = 0; a < 3; ++a) diag2 += (smax[a] - smin[a]) * (smax[a] - smin[a]);
    uint32_t mask = 0;
    for (int b = 0; b < n_boxes; ++b) {
        for (int a = 0; a < 4; ++a) spheres[b][a] = 0.0f;
        if (!((want >> b) & 1u) || tri_box.size() != nt) continue;
        float c[3];
        double half2 = 0.0;                               // the half diagonal: the farthest box corner from c
        for (int a = 0; a < 3; ++a) {
            c[a] = (boxes[b][a] + boxes[b][3 + a]) * 0.5f;
            const double h = std::max(double(boxes[b][3 + a]) - c[a], double(c[a]) - boxes[b][a]);
            half2 += h * h;
        }
        double r2 = -1.0;
        for (size_t k = 0; k < nt; ++k) {
            if (tri_box[k] != b) continue;
            for (int j = 0; j < 3; ++j) {
                double d2 = 0.0;
                for (int a = 0; a < 3; ++a) {
                    const double d = double(hs.kd_verts[9 * k + 3 * j + a]) - c[a];
                    d2 += d * d;
                }
                r2 = std::max(r2, d2);
            }
        }
        if (!(r2 > 0.0) || !std::isfinite(r2) || !std::isfinite(half2)) continue;
        const double r = std::sqrt(r2) * (1.0 + margin);
        if (!(r * r < half2) || !(diag2 <= max_reach * max_reach * r * r)) continue;
        // radius^2 rounded up: the next fp32 at or above r * r (r already carries sqrt's rounding
        // under a margin 2^42 times larger)
        float r2f = static_cast<float>(r * r);
        if (double(r2f) < r * r) r2f = std::nextafter(r2f, INFINITY);
        if (!std::isfinite(r2f) || !std::isfinite(c[0]) || !std::isfinite(c[1]) || !std::isfinite(c[2])) continue;
        spheres[b][0] = c[0]; spheres[b][1] = c[1]; spheres[b][2] = c[2]; spheres[b][3] = r2f;
        mask |= 1u << b;
    }
    return mask;
}

// ---------------------------------------------------------------------------
// KD build (KDTree.hpp:58-287). Literal std::min/std::max forms keep the
// signed-zero/NaN behaviour of the reference; float expressions keep its
// operand order (the library is compiled with -ffp-contract=off).
namespace {

inline float smin(float a, float b) { return (b < a) ? b : a; }
inline float smax(float a, float b) { return (a < b) ? b : a; }

struct Box {
    float mn[3], mx[3];
    static Box empty() {
        Box b;
        for (int i = 0; i < 3; ++i) { b.mn[i] = FLT_MAX; b.mx[i] = -FLT_MAX; }
        return b;
    }
    void add_pt(const float* p) {
        for (int i = 0; i < 3; ++i) { mn[i] = smin(mn[i], p[i]); mx[i] = smax(mx[i], p[i]); }
    }
    void add(const Box& r) { add_pt(r.mn); add_pt(r.mx); }
    void clip(const Box& r) {
        for (int i = 0; i < 3; ++i) { mn[i] = smax(mn[i], r.mn[i]); mx[i] = smin(mx[i], r.mx[i]); }
    }
    float half_area() const {
        float s0 = mx[0] - mn[0], s1 = mx[1] - mn[1], s2 = mx[2] - mn[2];
        return s0 * s1 + s1 * s2 + s2 * s0;
    }
};

struct BNode {
    Box box;
    Box region;                  // kd_build SAH: the split-plane region (not clipped to the triangles)
    std::vector<uint32_t> ids;   // ascending (std::set<UINT>)
    uint32_t axis = 0;
    float split = 0.0f;
    int32_t left = -1, right = -1;
    int depth = 0;
};

// flat-on-plane -> left; min < v -> left; max > v -> right (KDTree.hpp:129-153)
template <typename FL, typename FR>
inline void classify(const Box& tb, int a, float v, FL&& to_left, FR&& to_right) {
    if (tb.mn[a] == tb.mx[a] && tb.mn[a] == v) {
        to_left();
    } else {
        if (tb.mn[a] < v) to_left();
        if (tb.mx[a] > v) to_right();
    }
}

// kd_build = MCPT_KD_BUILD_SAH (not the reference's rule): every node,
// whatever its size, takes the split of least surface-area cost with a
// traversal term -- cost = Ct + Ci (A_L n_L + A_R n_R) / A, against the
// leaf's Ci n (Wald & Havran, "On building fast kd-trees for ray tracing, and
// on doing that in O(N log N)", 2006; no empty-space bonus) -- where the areas
// are those of the node's split-plane REGION cut at the plane (the space the
// ordered walk's intervals cover; the reference's SAH uses the child boxes
// clipped to the triangles and Ct = 0, KDTree.hpp:166) and the candidates are
// the faces of the triangles' boxes strictly inside the region, so empty
// space can be cut off.  One sweep per axis over sorted box ends: candidates
// in ascending order per axis, axes 0..2, the first strict minimum wins (the
// oracle, oracle/kdtree_ref.c, restates exactly this).  Triangle classification,
// child boxes, depth cap and the BFS flatten are the reference's.  Priced on
// the C1 frame: inner visits -43%, leaf visits -42%, triangle tests -5%.
#ifndef MCPT_SAH_CT          // (A/B builds only; the oracle restates 1 and 1.5)
#define MCPT_SAH_CT 1.0f
#define MCPT_SAH_CI 1.5f
#endif
constexpr float kSahCt = MCPT_SAH_CT, kSahCi = MCPT_SAH_CI;
struct SahScratch {
    std::vector<float> mins, maxs, plan, cand;
};
bool sah_split(const std::vector<Box>& tbox, const std::vector<uint32_t>& ids, const Box& R, SahScratch& w,
               int& ax, float& val) {
    const float sz[3] = {R.mx[0] - R.mn[0], R.mx[1] - R.mn[1], R.mx[2] - R.mn[2]};
    const float A0 = sz[0] * sz[1] + sz[1] * sz[2] + sz[2] * sz[0];
    if (!(A0 > 0.0f)) return false;
    const size_t n = ids.size();
    float best = kSahCi * static_cast<float>(n);
    bool found = false;
    for (int a = 0; a < 3; ++a) {
        w.mins.clear(); w.maxs.clear(); w.plan.clear(); w.cand.clear();
        for (uint32_t id : ids) {
            const float lo = tbox[id].mn[a], hi = tbox[id].mx[a];
            w.mins.push_back(lo);
            w.maxs.push_back(hi);
            if (lo == hi) w.plan.push_back(lo);
            // (+ 0.0f: a -0 candidate becomes +0, one value whatever the sort order of equal keys)
            if (R.mn[a] < lo && lo < R.mx[a]) w.cand.push_back(lo + 0.0f);
            if (R.mn[a] < hi && hi < R.mx[a]) w.cand.push_back(hi + 0.0f);
        }
        std::sort(w.mins.begin(), w.mins.end());
        std::sort(w.maxs.begin(), w.maxs.end());
        std::sort(w.plan.begin(), w.plan.end());
        std::sort(w.cand.begin(), w.cand.end());
        size_t im = 0, ix = 0, ip = 0;
        for (size_t q = 0; q < w.cand.size(); ++q) {
            if (q > 0 && !(w.cand[q - 1] < w.cand[q])) continue;
            const float v = w.cand[q];
            while (im < n && w.mins[im] < v) ++im;             // min < v: left
            while (ix < n && !(v < w.maxs[ix])) ++ix;          // max <= v: not right
            while (ip < w.plan.size() && w.plan[ip] < v) ++ip;
            size_t jp = ip;
            while (jp < w.plan.size() && !(v < w.plan[jp])) ++jp;   // flat on the plane: left
            const float nL = static_cast<float>(im + (jp - ip)), nR = static_cast<float>(n - ix);
            float sL[3] = {sz[0], sz[1], sz[2]}, sR[3] = {sz[0], sz[1], sz[2]};
            sL[a] = v - R.mn[a];
            sR[a] = R.mx[a] - v;
            const float AL = sL[0] * sL[1] + sL[1] * sL[2] + sL[2] * sL[0];
            const float AR = sR[0] * sR[1] + sR[1] * sR[2] + sR[2] * sR[0];
            const float cost = kSahCt + kSahCi * ((AL * nL + AR * nR) / A0);
            if (cost < best) {
                best = cost;
                ax = a;
                val = v;
                found = true;
            }
        }
    }
    return found;
}

}  // namespace

void build_kdtree(const std::vector<float>& tv, std::vector<KdNode>& out,
                  std::vector<uint32_t>& leaf_ids, int& depth_out, int kd_build) {
    if (kd_build != MCPT_KD_BUILD_REFERENCE && kd_build != MCPT_KD_BUILD_SAH)
        throw Error{MCPT_E_INVALID, "unknown kd_build"};
    const size_t n = tv.size() / 9;
    std::vector<Box> tbox(n);
    for (size_t k = 0; k < n; ++k) {
        tbox[k] = Box::empty();
        for (int j = 0; j < 3; ++j) tbox[k].add_pt(&tv[9 * k + 3 * j]);
    }
    auto node_box = [&](const std::vector<uint32_t>& ids) {   // GetNodeAABB
        Box b = Box::empty();
        for (uint32_t id : ids) b.add(tbox[id]);
        return b;
    };

    std::vector<BNode> nodes;
    nodes.reserve(2 * n + 1);
    nodes.emplace_back();
    nodes[0].ids.resize(n);
    std::iota(nodes[0].ids.begin(), nodes[0].ids.end(), 0u);
    nodes[0].box = node_box(nodes[0].ids);
    nodes[0].region = nodes[0].box;
    std::deque<int32_t> work{0};
    SahScratch sah;
    int max_depth = 0;
    // The reference duplicates straddling triangles into both children down to
    // depth 32 (KDTree.hpp:103-153): triangles that straddle every split (long
    // slivers, a polygon fan) make that exponential -- the reference would
    // exhaust memory.  Budget: nodes and triangle references held by nodes
    // under construction stay within generous multiples of the input (the
    // bundled scenes and the 70k C4 mesh use <= 14 nodes and <= 15 references
    // per triangle); a build past it is refused instead of taking the host down.
    const uint64_t node_budget = std::max<uint64_t>(uint64_t(1) << 20, uint64_t(64) * n);
    const uint64_t ref_budget = std::max<uint64_t>(uint64_t(1) << 24, uint64_t(256) * n);
    uint64_t live_refs = n;

    struct Cand { float v; uint32_t ins; };
    std::vector<Cand> cands;

    while (!work.empty()) {
        const int32_t ni = work.front();
        work.pop_front();
        const int depth = nodes[ni].depth;
        max_depth = std::max(max_depth, depth);
        if (depth >= 32) continue;
        const Box box = nodes[ni].box;
        const std::vector<uint32_t>& ids = nodes[ni].ids;
        int ax = -1;
        float val = 0.0f;
        if (kd_build == MCPT_KD_BUILD_SAH) {
            if (!sah_split(tbox, ids, nodes[ni].region, sah, ax, val)) ax = -1;
        } else if (ids.size() > 64u) {
            // spatial median of the longest axis (KDTree.hpp:108-122)
            float sz[3] = {box.mx[0] - box.mn[0], box.mx[1] - box.mn[1], box.mx[2] - box.mn[2]};
            ax = 0;
            for (int i = 1; i < 3; ++i) if (sz[i] > sz[ax]) ax = i;
            val = 0.5f * (box.mx[ax] + box.mn[ax]);
        } else {
            // SAH over vertex coordinates, Cts = 0 (KDTree.hpp:164-285)
            const float A0 = box.half_area();
            const float SAH0 = static_cast<float>(ids.size());
            float minSAH = FLT_MAX;
            for (int a = 0; a < 3; ++a) {
                cands.clear();
                for (uint32_t id : ids)
                    for (int j = 0; j < 3; ++j)
                        cands.push_back({tv[9 * id + 3 * j + a], static_cast<uint32_t>(cands.size())});
                std::stable_sort(cands.begin(), cands.end(), [](const Cand& x, const Cand& y) { return x.v < y.v; });
                for (size_t q = 0; q < cands.size(); ++q) {
                    if (q > 0 && !(cands[q - 1].v < cands[q].v)) continue;   // std::set keeps the first
                    const float v = cands[q].v;
                    if (v < box.mn[a] || v > box.mx[a]) continue;
                    unsigned numL = 0, numR = 0;
                    Box bL = box, bR = box, tL = Box::empty(), tR = Box::empty();
                    bL.mx[a] = v;
                    bR.mn[a] = v;
                    for (uint32_t id : ids)
                        classify(tbox[id], a, v,
                                 [&] { ++numL; tL.add(tbox[id]); },
                                 [&] { ++numR; tR.add(tbox[id]); });
                    bL.clip(tL);
                    bR.clip(tR);
                    const float AL = bL.half_area(), AR = bR.half_area();
                    const float SAH = (AL * static_cast<float>(numL) + AR * static_cast<float>(numR)) / A0 + 0.0f;
                    if (SAH < minSAH) { minSAH = SAH; ax = a; val = v; }
                }
            }
            if (!(minSAH < SAH0)) ax = -1;
        }
        if (ax < 0) continue;   // leaf

        BNode l, r;
        l.box = box; l.box.mx[ax] = val;
        r.box = box; r.box.mn[ax] = val;
        l.region = nodes[ni].region; l.region.mx[ax] = val;
        r.region = nodes[ni].region; r.region.mn[ax] = val;
        for (uint32_t id : ids)
            classify(tbox[id], ax, val, [&] { l.ids.push_back(id); }, [&] { r.ids.push_back(id); });
        l.box.clip(node_box(l.ids));
        r.box.clip(node_box(r.ids));
        l.depth = r.depth = depth + 1;
        nodes[ni].axis = static_cast<uint32_t>(ax + 1);
        nodes[ni].split = val;
        nodes[ni].left = static_cast<int32_t>(nodes.size());
        nodes[ni].right = static_cast<int32_t>(nodes.size() + 1);
        live_refs += l.ids.size() + r.ids.size();
        live_refs -= nodes[ni].ids.size();
        std::vector<uint32_t>().swap(nodes[ni].ids);
        if (nodes.size() + 2 > node_budget || live_refs > ref_budget)
            throw Error{MCPT_E_UNSUPPORTED, "KD build exceeds its budget (" + std::to_string(nodes.size() + 2) +
                                                " nodes, " + std::to_string(live_refs) +
                                                " triangle references): straddling triangles duplicate without bound"};
        nodes.push_back(std::move(l));
        nodes.push_back(std::move(r));
        work.push_back(static_cast<int32_t>(nodes.size() - 2));
        work.push_back(static_cast<int32_t>(nodes.size() - 1));
    }

    // BFS flatten: children of a node land at consecutive BFS indices
    out.clear();
    out.reserve(nodes.size());
    leaf_ids.clear();
    std::deque<int32_t> bfs{0};
    while (!bfs.empty()) {
        const BNode& b = nodes[static_cast<size_t>(bfs.front())];
        bfs.pop_front();
        KdNode o;
        for (int i = 0; i < 3; ++i) { o.bmin[i] = b.box.mn[i]; o.bmax[i] = b.box.mx[i]; }
        if (b.axis) {
            o.left = static_cast<uint32_t>(out.size() + bfs.size() + 1);
            o.right = o.left + 1;
            o.axis = b.axis;
            o.split = b.split;
            bfs.push_back(b.left);
            bfs.push_back(b.right);
        } else {
            o.leaf_begin = static_cast<uint32_t>(leaf_ids.size());
            o.leaf_count = static_cast<uint32_t>(b.ids.size());
            leaf_ids.insert(leaf_ids.end(), b.ids.begin(), b.ids.end());
        }
        out.push_back(o);
    }
    depth_out = max_depth;
}

}  // namespace mcpt
