// kicp_map_files.hip -- the voxel map as a file: PCD v0.7, DATA binary (what mapping tools write and viewers read; no library
// needed).  Host code over the C-ABI of the map: save lists kicp_map_pointcloud, load re-inserts the points in file order - which
// reproduces every voxel's points in their order (the order of the voxels among themselves may differ; nothing a registration
// computes depends on it: the search visits the 27 neighbour voxels in a fixed order and the sums are exact).
#include <fstream>
#include <sstream>

#include "kicp_internal.hpp"

using namespace kicp;
using namespace kicp::host;

namespace {
struct PcdField {
    std::string name;
    size_t size = 0, count = 1, offset = 0;
    char type = '?';
};
struct PcdHeader {
    std::vector<PcdField> fields;
    bool has_size = false, has_type = false, has_width = false, has_height = false, has_points = false, has_params = false;
    unsigned long long width = 0, height = 1, points = 0;
    std::string data;
    double voxel_size = 0.0, max_distance = 0.0;
    unsigned int max_points_per_voxel = 0;
};
std::vector<std::string> words_of(const std::string &line) {
    std::istringstream in(line);
    std::vector<std::string> w;
    for (std::string t; in >> t;) w.push_back(t);
    return w;
}
// the header up to and including the DATA line: comment lines anywhere, the entries in any order
int read_header(std::istream &in, const std::string &path, PcdHeader &h) {
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line.back() == '\r') line.pop_back();
        if (line.rfind("# kicp_map", 0) == 0) {
            h.has_params = std::sscanf(line.c_str(), "# kicp_map voxel_size=%lf max_distance=%lf max_points_per_voxel=%u", &h.voxel_size, &h.max_distance,
                                       &h.max_points_per_voxel) == 3;
            continue;
        }
        const std::vector<std::string> w = words_of(line);
        if (w.empty() || w[0][0] == '#') continue;
        const size_t args = w.size() - 1;
        auto per_field = [&](const char *what) {
            if (h.fields.empty()) return fail(KICP_ERR_ARG, path + ": PCD header has " + what + " before FIELDS");
            if (args != h.fields.size()) return fail(KICP_ERR_ARG, path + ": PCD header: " + what + " lists " + std::to_string(args) + " entries for " + std::to_string(h.fields.size()) + " fields");
            return static_cast<int>(KICP_OK);
        };
        if (w[0] == "FIELDS") {
            h.fields.resize(args);
            for (size_t i = 0; i < args; ++i) h.fields[i].name = w[i + 1];
        } else if (w[0] == "SIZE") {
            if (int rc = per_field("SIZE")) return rc;
            for (size_t i = 0; i < args; ++i) h.fields[i].size = std::strtoull(w[i + 1].c_str(), nullptr, 10);
            h.has_size = true;
        } else if (w[0] == "TYPE") {
            if (int rc = per_field("TYPE")) return rc;
            for (size_t i = 0; i < args; ++i) h.fields[i].type = w[i + 1][0];
            h.has_type = true;
        } else if (w[0] == "COUNT") {
            if (int rc = per_field("COUNT")) return rc;
            for (size_t i = 0; i < args; ++i) h.fields[i].count = std::strtoull(w[i + 1].c_str(), nullptr, 10);
        } else if (w[0] == "WIDTH" && args == 1) {
            h.width = std::strtoull(w[1].c_str(), nullptr, 10), h.has_width = true;
        } else if (w[0] == "HEIGHT" && args == 1) {
            h.height = std::strtoull(w[1].c_str(), nullptr, 10), h.has_height = true;
        } else if (w[0] == "POINTS" && args == 1) {
            h.points = std::strtoull(w[1].c_str(), nullptr, 10), h.has_points = true;
        } else if (w[0] == "DATA") {
            h.data = args ? w[1] : "";
            return KICP_OK;
        }  // (VERSION, VIEWPOINT and anything unknown: skipped)
    }
    return fail(KICP_ERR_ARG, path + ": not a PCD file (no DATA line)");
}
}  // namespace

extern "C" {

int kicp_map_params(const kicp_map *map, double *out_voxel_size, double *out_max_distance, unsigned int *out_max_points_per_voxel) {
    if (!map) return fail(KICP_ERR_ARG, "null map");
    if (out_voxel_size) *out_voxel_size = map->host.voxel_size();
    if (out_max_distance) *out_max_distance = map->host.max_distance();
    if (out_max_points_per_voxel) *out_max_points_per_voxel = static_cast<unsigned int>(map->host.cap());
    return KICP_OK;
}
int kicp_map_save_pcd(const kicp_map *cmap, const char *path) {
    KICP_TRACE_CALL();
    if (!cmap || !path) return fail(KICP_ERR_ARG, "null argument");
    kicp_map *map = const_cast<kicp_map *>(cmap);  // logically const, as kicp_map_pointcloud
    if (int rc = map_finish_pending(map)) return rc;  // (its error is this call's: the map it would write is not the updated one)
    const size_t n = kicp_map_num_points(map);
    std::vector<double> xyz(3 * n);
    if (n && kicp_map_pointcloud(map, xyz.data(), n) != n) return fail(KICP_ERR_HIP, "kicp_map_save_pcd: the map could not be listed");
    const std::string tmp = std::string(path) + ".tmp";
    std::FILE *f = std::fopen(tmp.c_str(), "wb");
    if (!f) return fail(KICP_ERR_ARG, "cannot write " + tmp + ": " + std::strerror(errno));
    bool ok = std::fprintf(f,
                           "# .PCD v0.7 - Point Cloud Data file format\n"
                           "# kicp_map voxel_size=%.17g max_distance=%.17g max_points_per_voxel=%u\n"
                           "VERSION 0.7\nFIELDS x y z\nSIZE 8 8 8\nTYPE F F F\nCOUNT 1 1 1\nWIDTH %zu\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %zu\nDATA binary\n",
                           map->host.voxel_size(), map->host.max_distance(), static_cast<unsigned int>(map->host.cap()), n, n) > 0;
    ok = ok && std::fwrite(xyz.data(), sizeof(double), xyz.size(), f) == xyz.size();
    ok = (std::fclose(f) == 0) && ok;
    if (!ok || std::rename(tmp.c_str(), path) != 0) {
        const std::string why = std::strerror(errno);
        std::remove(tmp.c_str());
        return fail(KICP_ERR_ARG, std::string("cannot write ") + path + ": " + why);
    }
    return KICP_OK;
}

int kicp_map_load_pcd(const char *path, double voxel_size, double max_distance, unsigned int max_points_per_voxel, int device, kicp_map **out,
                      size_t *out_points_read, size_t *out_points_dropped) {
    KICP_TRACE_CALL();
    if (!path || !out) return fail(KICP_ERR_ARG, "null argument");
    *out = nullptr;
    if (out_points_read) *out_points_read = 0;
    if (out_points_dropped) *out_points_dropped = 0;
    const std::string name(path);
    std::ifstream in(name, std::ios::binary);
    if (!in) return fail(KICP_ERR_ARG, "cannot read " + name);
    PcdHeader h;
    if (int rc = read_header(in, name, h)) return rc;
    if (h.data != "binary") return fail(KICP_ERR_ARG, name + ": DATA " + h.data + " is not supported (DATA binary only)");
    if (h.fields.empty() || !h.has_size || !h.has_type) return fail(KICP_ERR_ARG, name + ": PCD header lacks FIELDS, SIZE or TYPE");
    const PcdField *axis[3] = {nullptr, nullptr, nullptr};
    size_t stride = 0;
    for (PcdField &f : h.fields) {
        f.offset = stride, stride += f.size * f.count;
        for (int a = 0; a < 3; ++a)
            if (f.name == std::string(1, "xyz"[a]) && !axis[a]) axis[a] = &f;
    }
    for (int a = 0; a < 3; ++a) {
        const std::string field(1, "xyz"[a]);
        if (!axis[a]) return fail(KICP_ERR_ARG, name + ": PCD file has no field " + field);
        if (axis[a]->type != 'F' || (axis[a]->size != 4 && axis[a]->size != 8) || axis[a]->count != 1)
            return fail(KICP_ERR_ARG, name + ": field " + field + " must be TYPE F, SIZE 4 or 8, COUNT 1");
    }
    if (!h.has_points && !h.has_width) return fail(KICP_ERR_ARG, name + ": PCD header lacks POINTS and WIDTH");
    const unsigned long long points = h.has_points ? h.points : h.width * h.height;
    if (voxel_size <= 0.0) {  // the three parameters from the file
        if (!h.has_params) return fail(KICP_ERR_ARG, name + ": no '# kicp_map' line: pass voxel_size, max_distance and max_points_per_voxel");
        voxel_size = h.voxel_size, max_distance = h.max_distance, max_points_per_voxel = h.max_points_per_voxel;
    }
    // the rows, a piece at a time; non-finite points are dropped (and counted), the others keep the file's order
    std::vector<double> xyz;
    xyz.reserve(static_cast<size_t>(std::min<unsigned long long>(points, 1ull << 24)) * 3);
    const size_t piece_rows = std::max<size_t>(1, (4u << 20) / std::max<size_t>(stride, 1));
    std::vector<char> piece(piece_rows * stride);
    size_t dropped = 0;
    for (unsigned long long done = 0; done < points;) {
        const size_t rows = static_cast<size_t>(std::min<unsigned long long>(piece_rows, points - done));
        in.read(piece.data(), static_cast<std::streamsize>(rows * stride));
        const size_t got = static_cast<size_t>(in.gcount()) / stride;
        if (got < rows)
            return fail(KICP_ERR_ARG, name + ": truncated: the header announces " + std::to_string(points) + " points, the data holds " + std::to_string(done + got));
        for (size_t r = 0; r < rows; ++r) {
            double p[3];
            for (int a = 0; a < 3; ++a) {
                const char *at = piece.data() + r * stride + axis[a]->offset;
                if (axis[a]->size == 8) {
                    std::memcpy(&p[a], at, 8);
                } else {
                    float v;
                    std::memcpy(&v, at, 4);
                    p[a] = static_cast<double>(v);
                }
            }
            if (std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2])) xyz.insert(xyz.end(), p, p + 3);
            else ++dropped;
        }
        done += rows;
    }
    kicp_map *map = nullptr;
    if (int rc = kicp_map_create(voxel_size, max_distance, max_points_per_voxel, &map)) return rc;
    int rc = device >= 0 ? kicp_map_set_device(map, device) : KICP_OK;  // bulk insertion on that device; otherwise on the host
    if (rc == KICP_OK) rc = kicp_map_add_points(map, xyz.data(), xyz.size() / 3);
    if (rc != KICP_OK) {
        kicp_map_destroy(map);
        return rc;
    }
    *out = map;
    if (out_points_read) *out_points_read = static_cast<size_t>(points);
    if (out_points_dropped) *out_points_dropped = dropped;
    return KICP_OK;
}

}  // extern "C"
