// gol-mi355x: Python bindings (pybind11) — module `_gol`.
//
// Exposes the native framework to the Python package (game-of-life---mpi-cuda_amd/): geometry,
// patterns, the work planner, transports (including a callback transport driven by
// torch.distributed / gloo), the Engine, dump formatting, the CLI driver and benchmark helpers.
// Engine.run releases the GIL; the callback transport re-acquires it for each call.
#include <pybind11/functional.h>
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>

#include "gol/bench.hpp"
#include "gol/bits.hpp"
#include "gol/config.hpp"
#include "gol/cpu.hpp"
#include "gol/engine.hpp"
#include "gol/hip_kernels.hpp"
#include "gol/io.hpp"
#include "gol/pattern.hpp"
#include "gol/plan.hpp"
#include "gol/rle.hpp"
#include "gol/runtime.hpp"
#include "gol/soups.hpp"
#include "gol/transport.hpp"

namespace py = pybind11;
using namespace gol;

namespace {

// Transport whose primitives are Python callables (used with torch.distributed gloo on CPU).
//   send(peer, memoryview)              blocking, per-pair FIFO
//   recv(peer, memoryview)              fills the memoryview in place
//   exchange(sends, recvs) [optional]   lists of (peer, memoryview); must not deadlock
//   barrier() [optional]
class PyTransport : public Transport {
   public:
    PyTransport(int rank, int size, py::function send, py::function recv, py::object exchange, py::object barrier)
        : rank_(rank), size_(size), send_(std::move(send)), recv_(std::move(recv)), exch_(std::move(exchange)),
          barrier_(std::move(barrier)) {}
    ~PyTransport() override {
        py::gil_scoped_acquire g;
        send_ = py::function();
        recv_ = py::function();
        exch_ = py::object();
        barrier_ = py::object();
    }
    int rank() const override { return rank_; }
    int size() const override { return size_; }
    std::string name() const override { return "python"; }
    void send_bytes(int peer, const void* buf, size_t n) override {
        py::gil_scoped_acquire g;
        send_(peer, py::memoryview::from_memory(const_cast<void*>(buf), (ssize_t)n, true));
    }
    void recv_bytes(int peer, void* buf, size_t n) override {
        py::gil_scoped_acquire g;
        recv_(peer, py::memoryview::from_memory(buf, (ssize_t)n, false));
    }
    void exchange(const std::vector<Message>& sends, const std::vector<Message>& recvs, void* s) override {
        py::gil_scoped_acquire g;
        if (exch_.is_none()) {
            py::gil_scoped_release r;
            Transport::exchange(sends, recvs, s);
            return;
        }
        py::list ls, lr;
        for (const Message& m : sends) ls.append(py::make_tuple(m.peer, py::memoryview::from_memory(m.buf, (ssize_t)m.bytes, true)));
        for (const Message& m : recvs) lr.append(py::make_tuple(m.peer, py::memoryview::from_memory(m.buf, (ssize_t)m.bytes, false)));
        exch_(ls, lr);
    }
    void barrier() override {
        {
            py::gil_scoped_acquire g;
            if (!barrier_.is_none()) {
                barrier_();
                return;
            }
        }
        Transport::barrier();
    }

   private:
    int rank_, size_;
    py::function send_, recv_;
    py::object exch_, barrier_;
};

py::array_t<u64> words_to_numpy(const std::vector<u64>& w, i64 rows, i64 nw) {
    py::array_t<u64> a({(py::ssize_t)rows, (py::ssize_t)nw});
    std::memcpy(a.mutable_data(), w.data(), w.size() * 8);
    return a;
}

// A dense-cell call on (data_ptr, type code, numel), without the GIL; a gol::Error becomes a ValueError.
template <typename F>
void cells_call(F f, uintptr_t ptr, int code, i64 numel) {
    try {
        const CellBuffer b{reinterpret_cast<void*>(ptr), cell_type_from_code(code), numel};
        py::gil_scoped_release r;
        f(b);
    } catch (const Error& e) {
        throw py::value_error(e.what());
    }
}

py::dict stats_dict(const EngineStats& s) {
    py::dict d;
    d["generations"] = s.generations;
    d["supersteps"] = s.supersteps;
    d["exchanges"] = s.exchanges;
    d["halo_bytes"] = s.halo_bytes;
    d["graph_launches"] = s.graph_launches;
    d["depth"] = s.depth;
    d["plan_waves"] = s.plan_waves;
    d["lane_efficiency"] = s.lane_efficiency;
    d["predicted_us_per_gen"] = s.predicted_us_per_gen;
    d["predicted_gens"] = s.predicted_gens;
    d["t_exchange_ms"] = s.t_exchange_ms;
    d["t_compute_ms"] = s.t_compute_ms;
    d["kernel"] = s.kernel;
    d["rule"] = s.rule;
    d["states"] = s.states;
    d["boundary"] = s.boundary;
    d["census"] = s.census;
    d["signature"] = s.signature;
    if (s.film.on)
        d["film"] = py::make_tuple(s.film.r0, s.film.c0, s.film.rows, s.film.cols);
    else
        d["film"] = py::none();
    if (s.density_film.on)
        d["density_film"] = py::make_tuple(s.density_film.rows, s.density_film.cols);
    else
        d["density_film"] = py::none();
    if (s.envelope)
        d["envelope"] = s.envelope_start;
    else
        d["envelope"] = py::none();
    d["schedule"] = s.schedule;
    d["kernel_depth"] = s.kernel_depth;
    d["tile_waves"] = s.tile_waves;
    d["tuning"] = s.tuning;
    d["registered"] = s.registered;
    d["view_bytes_d2h"] = s.view_bytes_d2h;
    d["match_launches"] = s.match_launches;
    return d;
}

// a template's value or care cells as a (th, tw) uint8 array
py::array_t<u8> template_cells(const MatchTemplate& t, bool care) {
    py::array_t<u8> a({(py::ssize_t)t.th, (py::ssize_t)t.tw});
    u8* p = a.mutable_data();
    for (int i = 0; i < t.th; ++i)
        for (int j = 0; j < t.tw; ++j) p[i * t.tw + j] = (u8)(care ? t.cell_care(i, j) : t.cell_value(i, j));
    return a;
}

// ComponentsResult as (count, board (k,), anchor (k, 2), population (k,), bbox (k, 4), hash (k,) or empty, truncated,
// per_board)
py::tuple components_tuple(const ComponentsResult& r) {
    const py::ssize_t k = (py::ssize_t)r.population.size();
    py::array_t<i64> board(k), anchor({k, (py::ssize_t)2}), bbox({k, (py::ssize_t)4});
    py::array_t<u32> pop(k), per((py::ssize_t)r.per_board.size());
    py::array_t<u64> hash((py::ssize_t)r.hash.size());
    if (k) {
        std::memcpy(board.mutable_data(), r.board.data(), (size_t)k * sizeof(i64));
        std::memcpy(anchor.mutable_data(), r.anchor.data(), (size_t)k * 2 * sizeof(i64));
        std::memcpy(bbox.mutable_data(), r.bbox.data(), (size_t)k * 4 * sizeof(i64));
        std::memcpy(pop.mutable_data(), r.population.data(), (size_t)k * sizeof(u32));
    }
    if (!r.hash.empty()) std::memcpy(hash.mutable_data(), r.hash.data(), r.hash.size() * sizeof(u64));
    if (!r.per_board.empty()) std::memcpy(per.mutable_data(), r.per_board.data(), r.per_board.size() * sizeof(u32));
    return py::make_tuple(r.count, board, anchor, pop, bbox, hash, r.truncated, per);
}

}  // namespace

PYBIND11_MODULE(_gol, m) {
    m.doc() = "gol-mi355x native core (gfx950 HIP kernels, RCCL halo exchange, CPU backend)";

    py::register_exception<ContractError>(m, "ContractError");
    py::register_exception<Error>(m, "GolError");

    // ---- geometry -------------------------------------------------------------------------
    py::class_<Decomposition>(m, "Decomposition")
        .def_readonly("H", &Decomposition::H)
        .def_readonly("W", &Decomposition::W)
        .def_readonly("P", &Decomposition::P)
        .def_readonly("Px", &Decomposition::Px)
        .def_readonly("Py", &Decomposition::Py)
        .def_readonly("per_rank", &Decomposition::per_rank)
        .def_readonly("row_starts", &Decomposition::row_starts)
        .def_readonly("col_starts", &Decomposition::col_starts)
        .def_readonly("strip_starts", &Decomposition::strip_starts)
        .def("two_d", &Decomposition::two_d)
        .def("describe", &Decomposition::describe);
    m.def("make_decomposition", &make_decomposition, py::arg("N"), py::arg("P"), py::arg("global_mode") = false,
          py::arg("decomp") = "1d", py::arg("grid") = "", py::arg("width") = 0);

    py::class_<Geometry>(m, "Geometry")
        .def_readonly("dec", &Geometry::dec)
        .def_readonly("rank", &Geometry::rank)
        .def_readonly("cx", &Geometry::cx)
        .def_readonly("cy", &Geometry::cy)
        .def_readonly("row0", &Geometry::row0)
        .def_readonly("col0", &Geometry::col0)
        .def_readonly("h", &Geometry::h)
        .def_readonly("w", &Geometry::w)
        .def_property_readonly("nbr", [](const Geometry& g) { return std::vector<int>(g.nbr.begin(), g.nbr.end()); });
    m.def("make_geometry", &make_geometry);

    py::class_<Layout>(m, "Layout")
        .def(py::init<i64, i64, int>())
        .def_readonly("h", &Layout::h)
        .def_readonly("w", &Layout::w)
        .def_readonly("nw", &Layout::nw)
        .def_readonly("R", &Layout::R)
        .def_readonly("pitch", &Layout::pitch);
    m.def("clamp_halo_depth", &clamp_halo_depth);

    // ---- patterns -------------------------------------------------------------------------
    py::enum_<Fill>(m, "Fill").value("Zero", Fill::Zero).value("Ones", Fill::Ones).value("Random", Fill::Random);
    py::class_<PatternSpec>(m, "PatternSpec")
        .def(py::init<>())
        .def_readwrite("pattern", &PatternSpec::pattern)
        .def_readwrite("seed", &PatternSpec::seed)
        .def_readwrite("fill", &PatternSpec::fill)
        .def_readwrite("cells", &PatternSpec::cells);
    m.def("make_pattern", &make_pattern, py::arg("pattern"), py::arg("dec"), py::arg("seed") = 0x5EED);
    m.def("random_word", &random_word);
    m.def("mix64", &mix64);

    // ---- planner --------------------------------------------------------------------------
    m.def(
        "build_plan",
        [](const std::vector<std::tuple<i64, i64, i64, i64>>& regions, i64 nw, i64 h, i64 rows, int k, bool xwrap,
           bool fold) {
            std::vector<Region> rg;
            for (auto& t : regions) rg.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)});
            PlanStats st;
            std::vector<LaneDesc> lanes = build_plan(rg, nw, h, rows, k, xwrap, &st, kWavesPerBlock, 8, fold);
            py::array_t<i32> a({(py::ssize_t)lanes.size(), (py::ssize_t)4});
            std::memcpy(a.mutable_data(), lanes.data(), lanes.size() * sizeof(LaneDesc));
            py::dict d;
            d["waves"] = st.waves;
            d["active_lanes"] = st.active_lanes;
            d["lane_rows"] = st.lane_rows;
            d["out_words"] = st.out_words;
            return py::make_tuple(a, d);
        },
        py::arg("regions"), py::arg("nw"), py::arg("h"), py::arg("rows_per_chunk"), py::arg("k"),
        py::arg("xwrap") = false, py::arg("fold") = false);
    m.def("choose_rows_per_chunk", [](const std::vector<std::tuple<i64, i64, i64, i64>>& regions, int k, i64 target,
                                      i64 min_rows) {
        std::vector<Region> rg;
        for (auto& t : regions) rg.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)});
        return choose_rows_per_chunk(rg, k, target, min_rows);
    });
    m.def(
        "balanced_rows_per_chunk",
        [](const std::vector<std::tuple<i64, i64, i64, i64>>& regions, i64 nw, i64 h, int k, i64 resident_waves,
           i64 min_rows, bool xwrap) {
            std::vector<Region> rg;
            for (auto& t : regions) rg.push_back({std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)});
            return balanced_rows_per_chunk(rg, nw, h, k, resident_waves, min_rows, xwrap);
        },
        py::arg("regions"), py::arg("nw"), py::arg("h"), py::arg("k"), py::arg("resident_waves"), py::arg("min_rows"),
        py::arg("xwrap") = false);

    // ---- transports -----------------------------------------------------------------------
    py::class_<Transport, std::shared_ptr<Transport>>(m, "Transport")
        .def("rank", &Transport::rank)
        .def("size", &Transport::size)
        .def("name", &Transport::name)
        .def("device_buffers", &Transport::device_buffers)
        .def("data_plane_ranks", &Transport::data_plane_ranks)
        .def("barrier", &Transport::barrier, py::call_guard<py::gil_scoped_release>())
        .def("allreduce_max", &Transport::allreduce_max, py::call_guard<py::gil_scoped_release>())
        .def("allreduce_min", &Transport::allreduce_min, py::call_guard<py::gil_scoped_release>())
        .def("allreduce_sum", &Transport::allreduce_sum, py::call_guard<py::gil_scoped_release>());
    py::class_<SelfTransport, Transport, std::shared_ptr<SelfTransport>>(m, "SelfTransport").def(py::init<>());
    py::class_<ThreadTransport, Transport, std::shared_ptr<ThreadTransport>>(m, "ThreadTransport");
    m.def("make_thread_transports", [](int P) {
        auto g = make_thread_group(P);
        std::vector<std::shared_ptr<Transport>> v;
        for (int r = 0; r < P; ++r) v.push_back(std::make_shared<ThreadTransport>(g, r));
        return v;
    });
    m.def("make_p2p_transports", [](int P) {
        auto g = make_thread_group(P);
        std::vector<std::shared_ptr<Transport>> v;
        for (int r = 0; r < P; ++r) v.push_back(make_p2p_emulation_transport(std::make_shared<ThreadTransport>(g, r)));
        return v;
    });
    py::class_<PyTransport, Transport, std::shared_ptr<PyTransport>>(m, "PyTransport")
        .def(py::init<int, int, py::function, py::function, py::object, py::object>(), py::arg("rank"),
             py::arg("size"), py::arg("send"), py::arg("recv"), py::arg("exchange") = py::none(),
             py::arg("barrier") = py::none());
    m.def("make_tcp_transport", &make_tcp_transport, py::arg("rank"), py::arg("size"), py::arg("addr"),
          py::arg("port"), py::arg("timeout_s") = 120.0, py::call_guard<py::gil_scoped_release>());
    m.def("make_rccl_transport", &make_rccl_transport, py::call_guard<py::gil_scoped_release>());
    m.def(
        "make_rccl_transport_with_id",
        [](std::shared_ptr<Transport> ctl, py::bytes uid) {
            std::string s = uid;
            py::gil_scoped_release r;
            return make_rccl_transport_with_id(ctl, s);
        },
        py::arg("control"), py::arg("unique_id"));
    m.def("rccl_unique_id", []() { return py::bytes(rccl_unique_id()); });

    // ---- engine ---------------------------------------------------------------------------
    py::class_<EngineConfig>(m, "EngineConfig")
        .def(py::init<>())
        .def_readwrite("backend", &EngineConfig::backend)
        .def_readwrite("halo_depth", &EngineConfig::halo_depth)
        .def_readwrite("overlap", &EngineConfig::overlap)
        .def_readwrite("graph", &EngineConfig::graph)
        .def_readwrite("compat", &EngineConfig::compat)
        .def_readwrite("device", &EngineConfig::device)
        .def_readwrite("rows_per_wave", &EngineConfig::rows_per_wave)
        .def_readwrite("waves_target", &EngineConfig::waves_target)
        .def_readwrite("kernel", &EngineConfig::kernel)
        .def_readwrite("transport", &EngineConfig::transport)
        .def_readwrite("profile", &EngineConfig::profile)
        .def_readwrite("graph_supersteps", &EngineConfig::graph_supersteps)
        .def_readwrite("run_hint", &EngineConfig::run_hint)
        .def_readwrite("subtiles", &EngineConfig::subtiles)
        .def_readwrite("watchdog_s", &EngineConfig::watchdog_s)
        .def_readwrite("tile_waves", &EngineConfig::tile_waves)
        .def_readwrite("tune_tile_waves", &EngineConfig::tune_tile_waves)
        .def_readwrite("sub_occ", &EngineConfig::sub_occ)
        .def_readwrite("subtile_overlap", &EngineConfig::subtile_overlap)
        .def_readwrite("self_exchange", &EngineConfig::self_exchange)
        .def_readwrite("force_split", &EngineConfig::force_split)
        .def_readwrite("sched", &EngineConfig::sched)
        .def_readwrite("kernel_depth", &EngineConfig::kernel_depth)
        .def_readwrite("graph_rccl", &EngineConfig::graph_rccl)
        .def_readwrite("plan_xcds", &EngineConfig::plan_xcds)
        .def_readwrite("census", &EngineConfig::census)
        .def_readwrite("signature", &EngineConfig::signature)
        // film mode: None (off) or the window (r0, c0, rows, cols)
        .def_property(
            "film",
            [](const EngineConfig& c) -> py::object {
                if (!c.film.on) return py::none();
                return py::make_tuple(c.film.r0, c.film.c0, c.film.rows, c.film.cols);
            },
            [](EngineConfig& c, py::object v) {
                if (v.is_none()) {
                    c.film = FilmRect();
                    return;
                }
                if (!py::isinstance<py::sequence>(v) || py::len(v) != 4) throw py::value_error("film must be None or (r0, c0, rows, cols)");
                const py::sequence q = py::reinterpret_borrow<py::sequence>(v);
                c.film = FilmRect{true, q[0].cast<i64>(), q[1].cast<i64>(), q[2].cast<i64>(), q[3].cast<i64>()};
            })
        .def_readwrite("envelope", &EngineConfig::envelope)
        // density-film mode: None (off) or the blocks (block_rows, block_cols)
        .def_property(
            "density_film",
            [](const EngineConfig& c) -> py::object {
                if (!c.density_film.on) return py::none();
                return py::make_tuple(c.density_film.rows, c.density_film.cols);
            },
            [](EngineConfig& c, py::object v) {
                if (v.is_none()) {
                    c.density_film = DensityBlocks();
                    return;
                }
                if (!py::isinstance<py::sequence>(v) || py::len(v) != 2)
                    throw py::value_error("density_film must be None or (block_rows, block_cols)");
                const py::sequence q = py::reinterpret_borrow<py::sequence>(v);
                c.density_film = DensityBlocks{true, q[0].cast<i64>(), q[1].cast<i64>()};
            })
        // the life-like rule as a string (any form Rule::parse takes; reads back canonical, B3/S23)
        .def_property(
            "rule", [](const EngineConfig& c) { return c.rule.str(); },
            [](EngineConfig& c, const std::string& s) {
                try {
                    c.rule = Rule::parse(s);
                } catch (const Error& e) {
                    throw py::value_error(e.what());
                }
            })
        // the board's boundary: "torus" (default) or "dead" (a bounded board); any other value is a ValueError
        .def_property(
            "boundary", [](const EngineConfig& c) { return std::string(boundary_name(c.boundary)); },
            [](EngineConfig& c, const std::string& s) {
                try {
                    c.boundary = parse_boundary(s);
                } catch (const Error& e) {
                    throw py::value_error(e.what());
                }
            });
    // rule string -> (birth, survive): bit c of birth / survive = a dead / live cell with c live neighbours lives
    m.def("parse_rule", [](const std::string& s) {
        try {
            const Rule r = Rule::parse(s);
            return py::make_tuple((unsigned)r.birth, (unsigned)r.survive);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    // rule string -> (birth, survive, neighbourhood suffix): "" Moore, "V" von Neumann, "H" hexagonal
    m.def("parse_rule_nbhd", [](const std::string& s) {
        try {
            const Rule r = Rule::parse(s);
            return py::make_tuple((unsigned)r.birth, (unsigned)r.survive, std::string(nbhd_suffix(r.nbhd)));
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    // rule string -> its states: 2 for a life-like rule, C of a Generations rule B<digits>/S<digits>/C<n>
    m.def("parse_rule_states", [](const std::string& s) {
        try {
            return (int)Rule::parse(s).states;
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    // rule string -> (R, M, smin, smax, bmin, bmax) of a Larger than Life rule R<r>,C<c>,M<m>,S<a>..<b>,B<a>..<b>[,NM]
    // (or the alias bosco); None for a rule of another family; ValueError on a string Rule::parse refuses
    m.def("parse_ltl_rule", [](const std::string& s) -> py::object {
        try {
            const Rule r = Rule::parse(s);
            if (!r.ltl()) return py::none();
            return py::make_tuple((unsigned)r.range, (unsigned)r.middle, (unsigned)r.smin, (unsigned)r.smax, (unsigned)r.bmin,
                                  (unsigned)r.bmax);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    // the canonical form of a rule string (Rule::str())
    m.def("canonical_rule", [](const std::string& s) {
        try {
            return Rule::parse(s).str();
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    // an LtL rule's four thresholds on the box sum that includes the centre: (blo, bhi, slo, shi) (Rule::ltl_thresholds)
    m.def("ltl_thresholds", [](const std::string& s) {
        try {
            const Rule r = Rule::parse(s);
            if (!r.ltl()) throw Error("ltl_thresholds: rule " + r.str() + " is not a Larger than Life rule");
            const Rule::LtlThresholds t = r.ltl_thresholds();
            return py::make_tuple((unsigned)t.blo, (unsigned)t.bhi, (unsigned)t.slo, (unsigned)t.shi);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });

    py::class_<Engine>(m, "Engine")
        .def_static(
            "create",
            [](const Geometry& g, const EngineConfig& c, std::shared_ptr<Transport> t) {
                py::gil_scoped_release r;
                return Engine::create(g, c, t);
            },
            py::arg("geometry"), py::arg("config"), py::arg("transport"))
        .def("init", &Engine::init, py::call_guard<py::gil_scoped_release>())
        .def("run", &Engine::run, py::call_guard<py::gil_scoped_release>())
        .def("synchronize", &Engine::synchronize, py::call_guard<py::gil_scoped_release>())
        .def("gpu_idle", &Engine::gpu_idle)
        .def("tile_words",
             [](Engine& e) {
                 std::vector<u64> w;
                 {
                     py::gil_scoped_release r;
                     w = e.tile_words();
                 }
                 return words_to_numpy(w, e.layout().h, e.layout().nw);
             })
        .def("set_tile_words",
             [](Engine& e, py::array_t<u64, py::array::c_style | py::array::forcecast> a) {
                 std::vector<u64> w(a.data(), a.data() + a.size());
                 py::gil_scoped_release r;
                 e.set_tile_words(w);
             })
        .def("local_reduce", &Engine::local_reduce, py::call_guard<py::gil_scoped_release>())
        .def("population", &Engine::population, py::call_guard<py::gil_scoped_release>())
        .def("fingerprint", &Engine::fingerprint, py::call_guard<py::gil_scoped_release>())
        // census mode (collective): (start, counts), counts[i] the global population at generation start + 1 + i
        .def("census",
             [](Engine& e) {
                 std::pair<u64, std::vector<u64>> c;
                 {
                     py::gil_scoped_release r;
                     c = e.census();
                 }
                 py::array_t<u64> a((py::ssize_t)c.second.size());
                 if (!c.second.empty()) std::memcpy(a.mutable_data(), c.second.data(), c.second.size() * sizeof(u64));
                 return py::make_tuple(c.first, a);
             })
        .def("census_clear", &Engine::census_clear, py::call_guard<py::gil_scoped_release>())
        // signature mode (collective): (start, signatures, populations), entry i for generation start + 1 + i
        .def("signatures",
             [](Engine& e) {
                 Engine::SignatureSeries s;
                 {
                     py::gil_scoped_release r;
                     s = e.signatures();
                 }
                 py::array_t<u64> a((py::ssize_t)s.signatures.size()), b((py::ssize_t)s.populations.size());
                 if (!s.signatures.empty()) std::memcpy(a.mutable_data(), s.signatures.data(), s.signatures.size() * sizeof(u64));
                 if (!s.populations.empty()) std::memcpy(b.mutable_data(), s.populations.data(), s.populations.size() * sizeof(u64));
                 return py::make_tuple(s.start, a, b);
             })
        .def("signatures_clear", &Engine::signatures_clear, py::call_guard<py::gil_scoped_release>())
        // film mode (collective): (start, frames), frames a (n, rows, cols) uint8 array, frame i the window at generation start + 1 + i
        .def("film",
             [](Engine& e) {
                 size_t n = 0;
                 {
                     py::gil_scoped_release r;
                     n = e.film_frames();
                 }
                 const FilmRect& w = e.config().film;
                 py::array_t<u8> a({(py::ssize_t)n, (py::ssize_t)w.rows, (py::ssize_t)w.cols});  // (unpacked in place)
                 u8* out = a.mutable_data();
                 u64 start = 0;
                 {
                     py::gil_scoped_release r;
                     start = e.film_into(out, n);
                 }
                 return py::make_tuple(start, a);
             })
        .def("film_clear", &Engine::film_clear, py::call_guard<py::gil_scoped_release>())
        // density-film mode (collective): (start, maps), maps a (n, grid_rows, grid_cols) uint32 array, map i the density grid
        // at generation start + 1 + i
        .def("density_film",
             [](Engine& e) {
                 size_t n = 0;
                 {
                     py::gil_scoped_release r;
                     n = e.density_film_frames();
                 }
                 const DensityGeo& g = e.density_geo();
                 py::array_t<u32> a({(py::ssize_t)n, (py::ssize_t)g.grid_rows, (py::ssize_t)g.grid_cols});  // (summed in place)
                 u32* out = a.mutable_data();
                 u64 start = 0;
                 {
                     py::gil_scoped_release r;
                     start = e.density_film_into(out, n);
                 }
                 return py::make_tuple(start, a);
             })
        .def("density_film_clear", &Engine::density_film_clear, py::call_guard<py::gil_scoped_release>())
        // envelope mode: (start, words), the OR of this rank's tile over generations start .. generation() as tile_words()
        // returns the board; the board's collective readers on the envelope; the reset
        .def("envelope",
             [](Engine& e) {
                 std::vector<u64> d;
                 u64 start = 0;
                 {
                     py::gil_scoped_release r;
                     start = e.envelope_start();
                     d = e.envelope_tile_words();
                 }
                 return py::make_tuple(start, words_to_numpy(d, e.layout().h, e.layout().nw));
             })
        .def("envelope_window",
             [](Engine& e, i64 r0, i64 c0, i64 rows, i64 cols) {
                 std::vector<u8> d;
                 {
                     py::gil_scoped_release r;
                     d = e.envelope_window(r0, c0, rows, cols);
                 }
                 py::array_t<u8> a({(py::ssize_t)rows, (py::ssize_t)cols});
                 memcpy(a.mutable_data(), d.data(), d.size());
                 return a;
             })
        .def("envelope_density",
             [](Engine& e, i64 block_rows, i64 block_cols) {
                 std::vector<u32> d;
                 {
                     py::gil_scoped_release r;
                     d = e.envelope_density(block_rows, block_cols);
                 }
                 const Decomposition& dec = e.geometry().dec;
                 py::array_t<u32> a({(py::ssize_t)ceil_div(dec.H, block_rows), (py::ssize_t)ceil_div(dec.W, block_cols)});
                 memcpy(a.mutable_data(), d.data(), d.size() * sizeof(u32));
                 return a;
             })
        .def("envelope_population", &Engine::envelope_population, py::call_guard<py::gil_scoped_release>())
        .def("envelope_clear", &Engine::envelope_clear, py::call_guard<py::gil_scoped_release>())
        // any mode (collective): the signature of the current board; a copy of the board, and the cells that differ from it
        .def("signature", &Engine::signature, py::call_guard<py::gil_scoped_release>())
        .def("snapshot", &Engine::snapshot, py::call_guard<py::gil_scoped_release>())
        .def("snapshot_diff", &Engine::snapshot_diff, py::call_guard<py::gil_scoped_release>())
        // Generations rules: the states of the tile (h, w) uint8, the reverse, the states of a window, the C counts;
        // what a call refuses (a two-state rule, a value >= C) is a ValueError
        .def_property_readonly("states", &Engine::states)
        .def("state_tile",
             [](Engine& e) {
                 std::vector<u8> v;
                 try {
                     py::gil_scoped_release r;
                     v = e.state_tile();
                 } catch (const Error& err) {
                     throw py::value_error(err.what());
                 }
                 py::array_t<u8> a({(py::ssize_t)e.layout().h, (py::ssize_t)e.layout().w});
                 std::memcpy(a.mutable_data(), v.data(), v.size());
                 return a;
             })
        .def("set_state_tile",
             [](Engine& e, py::array_t<u8, py::array::c_style | py::array::forcecast> a) {
                 std::vector<u8> v(a.data(), a.data() + a.size());
                 try {
                     py::gil_scoped_release r;
                     e.set_state_tile(v);
                 } catch (const Error& err) {
                     throw py::value_error(err.what());
                 }
             })
        .def(
            "state_window",
            [](Engine& e, i64 r0, i64 c0, i64 rows, i64 cols) {
                std::vector<u8> v;
                try {
                    py::gil_scoped_release r;
                    v = e.state_window(r0, c0, rows, cols);
                } catch (const Error& err) {
                    throw py::value_error(err.what());
                }
                py::array_t<u8> a({(py::ssize_t)rows, (py::ssize_t)cols});
                std::memcpy(a.mutable_data(), v.data(), v.size());
                return a;
            },
            py::arg("r0"), py::arg("c0"), py::arg("rows"), py::arg("cols"))
        .def("state_counts",
             [](Engine& e) {
                 std::vector<u64> v;
                 try {
                     py::gil_scoped_release r;
                     v = e.state_counts();
                 } catch (const Error& err) {
                     throw py::value_error(err.what());
                 }
                 py::array_t<u64> a((py::ssize_t)v.size());
                 std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(u64));
                 return a;
             })
        // views and stamping (collective; global board coordinates on the torus)
        .def(
            "window",
            [](Engine& e, i64 r0, i64 c0, i64 rows, i64 cols) {
                std::vector<u8> v;
                {
                    py::gil_scoped_release r;
                    v = e.window(r0, c0, rows, cols);
                }
                py::array_t<u8> a({(py::ssize_t)rows, (py::ssize_t)cols});
                std::memcpy(a.mutable_data(), v.data(), v.size());
                return a;
            },
            py::arg("r0"), py::arg("c0"), py::arg("rows"), py::arg("cols"))
        .def(
            "density",
            [](Engine& e, i64 block_rows, i64 block_cols) {
                std::vector<u32> v;
                {
                    py::gil_scoped_release r;
                    v = e.density(block_rows, block_cols);
                }
                const Decomposition& d = e.geometry().dec;
                py::array_t<u32> a({(py::ssize_t)ceil_div(d.H, block_rows), (py::ssize_t)ceil_div(d.W, block_cols)});
                std::memcpy(a.mutable_data(), v.data(), v.size() * sizeof(u32));
                return a;
            },
            py::arg("block_rows"), py::arg("block_cols"))
        .def(
            "stamp",
            [](Engine& e, const RlePattern& p, i64 r0, i64 c0, const std::string& mode) {
                const StampMode m = parse_stamp_mode(mode);
                py::gil_scoped_release r;
                e.stamp(p, r0, c0, m);
            },
            py::arg("pattern"), py::arg("r0"), py::arg("c0"), py::arg("mode") = "or")
        // dense cells (gol/cells.hpp): (data_ptr, element type code 0 u8 / 1 f16 / 2 bf16 / 3 f32, numel) of a caller's
        // buffer, device memory on the HIP backend and host memory on the CPU backend; what a call refuses is a ValueError
        .def("read_tile_cells", [](Engine& e, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& b) { e.read_tile_cells(b); }, ptr, code, numel);
        })
        .def("read_envelope_cells", [](Engine& e, uintptr_t ptr, int code, i64 numel) {
            u64 start = 0;
            cells_call([&](const CellBuffer& b) {
                start = e.envelope_start();
                e.read_envelope_cells(b);
            }, ptr, code, numel);
            return start;
        })
        .def("write_tile_cells", [](Engine& e, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& b) { e.write_tile_cells(b); }, ptr, code, numel);
        })
        .def("read_window_cells", [](Engine& e, i64 r0, i64 c0, i64 rows, i64 cols, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& b) { e.read_window_cells(r0, c0, rows, cols, b); }, ptr, code, numel);
        })
        .def("run_film_cells", [](Engine& e, u64 generations, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& b) { e.run_film_cells(generations, b); }, ptr, code, numel);
        })
        // pattern matching (gol/match.hpp): ts = [(orientation id, MatchTemplate)]; (count, positions (k, 2) int64, orientation
        // (k,) uint8, truncated); what a call refuses is a ValueError, raised before anything is launched
        .def(
            "match",
            [](Engine& e, const std::vector<std::pair<int, MatchTemplate>>& ts, i64 max_hits, bool positions) {
                Engine::MatchResult res;
                try {
                    py::gil_scoped_release r;
                    res = e.match(ts, max_hits, positions);
                } catch (const Error& err) {
                    throw py::value_error(err.what());
                }
                const py::ssize_t k = (py::ssize_t)res.orientation.size();
                py::array_t<i64> pos({k, (py::ssize_t)2});
                py::array_t<u8> ids(k);
                for (py::ssize_t i = 0; i < 2 * k; ++i) pos.mutable_data()[i] = res.positions[(size_t)i];
                if (k) std::memcpy(ids.mutable_data(), res.orientation.data(), (size_t)k);
                return py::make_tuple(res.count, pos, ids, res.truncated);
            },
            py::arg("templates"), py::arg("max_hits") = (i64)1 << 20, py::arg("positions") = true)
        .def("match_cells", [](Engine& e, const std::vector<std::pair<int, MatchTemplate>>& ts, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& b) { e.match_cells(ts, b); }, ptr, code, numel);
        })
        // connected components (gol/components.hpp): components_tuple(); what a call refuses is a ValueError, raised before
        // anything is launched
        .def(
            "components",
            [](Engine& e, const std::string& neighbourhood, i64 max_objects, bool hashes, bool records) {
                ComponentsResult res;
                try {
                    const CcNeighbourhood nb = cc_neighbourhood(neighbourhood);
                    py::gil_scoped_release r;
                    res = e.components(nb, max_objects, hashes, records);
                } catch (const Error& err) {
                    throw py::value_error(err.what());
                }
                return components_tuple(res);
            },
            py::arg("neighbourhood") = "moore", py::arg("max_objects") = (i64)1 << 20, py::arg("hashes") = true,
            py::arg("records") = true)
        // (h, w) labels into the int32 or int64 buffer at ptr
        .def("components_labels", [](Engine& e, const std::string& neighbourhood, uintptr_t ptr, bool int64, i64 numel) {
            try {
                const CcNeighbourhood nb = cc_neighbourhood(neighbourhood);
                py::gil_scoped_release r;
                e.components_labels(nb, reinterpret_cast<void*>(ptr), int64, numel);
            } catch (const Error& err) {
                throw py::value_error(err.what());
            }
        })
        .def("device_barrier", &Engine::device_barrier, py::call_guard<py::gil_scoped_release>())
        .def("phase_probe", &Engine::phase_probe, py::arg("k"), py::call_guard<py::gil_scoped_release>())
        .def("time_runs", &Engine::time_runs, py::arg("gens"), py::arg("reps"), py::call_guard<py::gil_scoped_release>())
        .def_property_readonly("geometry", &Engine::geometry)
        .def_property_readonly("layout", &Engine::layout)
        .def_property_readonly("generation", &Engine::generation)
        .def("stats", [](const Engine& e) { return stats_dict(e.stats()); })
        .def("describe", &Engine::describe)
        .def("backend_name", &Engine::backend_name)
        .def("halo_items", [](const Engine& e, int k) {
            py::list l;
            for (const auto& it : e.halo_items(k))
                l.append(py::make_tuple(dir_name(it.d), it.send_peer, it.recv_peer,
                                        py::make_tuple(it.send.r0, it.send.rows, it.send.c0, it.send.words),
                                        py::make_tuple(it.recv.r0, it.recv.rows, it.recv.c0, it.recv.words),
                                        it.contiguous));
            return l;
        });
    m.def("write_dumps", [](Engine& e, const std::string& path) {
        FILE* f = fopen(path.c_str(), "w");
        if (!f) throw Error("cannot open " + path);
        {
            py::gil_scoped_release r;
            write_dumps(e, f);
        }
        fclose(f);
    });
    m.def("save_checkpoint", &save_checkpoint, py::call_guard<py::gil_scoped_release>());
    m.def("load_checkpoint", &load_checkpoint, py::call_guard<py::gil_scoped_release>());

    // ---- CPU oracle ---------------------------------------------------------------------------
    m.def(
        "cpu_torus_step",
        [](py::array_t<u64, py::array::c_style | py::array::forcecast> words, i64 w, int gens) {
            // Full-torus reference on dense packed words (h x nw) via the CPU backend.
            const i64 h = words.shape(0), nw = words.shape(1);
            Layout L(h, w, 1);
            std::vector<u64> a((size_t)L.words(), 0), b((size_t)L.words(), 0);
            cpu::insert_words(a.data(), L, words.data());
            u64* cur = a.data();
            u64* oth = b.data();
            {
                py::gil_scoped_release r;
                for (int g = 0; g < gens; ++g) {
                    cpu::fill_ghost_cols_wrap(cur, L, 0, L.h);
                    cpu::fill_ghost_rows_wrap(cur, L);
                    cpu::step_rows(cur, oth, L, 0, L.h);
                    std::swap(cur, oth);
                }
            }
            std::vector<u64> out((size_t)(h * nw));
            cpu::extract_words(cur, L, out.data());
            return words_to_numpy(out, h, nw);
        },
        py::arg("words"), py::arg("w"), py::arg("gens"));

    // ---- RLE patterns ---------------------------------------------------------------------
    py::class_<RlePattern>(m, "RlePattern")
        .def(py::init([](py::array_t<u64, py::array::c_style | py::array::forcecast> words, i64 cols, const std::string& rule,
                         const std::string& topology, i64 bound_cols, i64 bound_rows) {
                 if (words.ndim() != 2 || cols < 1 || words.shape(0) < 1 || words.shape(1) != ceil_div(cols, 64))
                     throw py::value_error("RlePattern: words must be a (rows, ceil(cols / 64)) uint64 array");
                 if (topology.empty() ? (bound_cols != 0 || bound_rows != 0)
                                      : ((topology != "T" && topology != "P") || bound_cols < 1 || bound_rows < 1))
                     throw py::value_error("RlePattern: topology is '', 'T' or 'P', with a board of >= 1 x 1 cells when set");
                 RlePattern p;
                 p.rows = words.shape(0);
                 p.cols = cols;
                 p.rule = rule;
                 p.topology = topology;
                 p.bound_cols = bound_cols;
                 p.bound_rows = bound_rows;
                 p.words.assign(words.data(), words.data() + words.size());
                 for (i64 r = 0; r < p.rows; ++r) p.words[(size_t)(r * p.nw() + p.nw() - 1)] &= word_mask(p.nw() - 1, cols);
                 return p;
             }),
             py::arg("words"), py::arg("cols"), py::arg("rule") = "", py::arg("topology") = "", py::arg("bound_cols") = 0,
             py::arg("bound_rows") = 0)
        .def_readonly("topology", &RlePattern::topology)
        .def_readonly("bound_cols", &RlePattern::bound_cols)
        .def_readonly("bound_rows", &RlePattern::bound_rows)
        .def_readonly("rows", &RlePattern::rows)
        .def_readonly("cols", &RlePattern::cols)
        .def_readonly("rule", &RlePattern::rule)
        .def_property_readonly("words", [](const RlePattern& p) { return words_to_numpy(p.words, p.rows, p.nw()); });
    // (a text or a file no reader accepts is a ValueError, like a bad rule string)
    m.def("parse_rle", [](const std::string& text) {
        try {
            return parse_rle(text);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    m.def("read_rle_file", [](const std::string& path) {
        try {
            return read_rle_file(path);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    });
    m.def("write_rle", &write_rle);
    m.def("write_rle_file", &write_rle_file);

    // measurement switch of tools/measure_components.py: components() on the HIP backends with (the default) or without
    // the reduction across a wave in k_cc_stats and k_cc_hash; the results do not depend on it
    m.def("cc_wave_reduce", [](bool on) { hipk::cc_set_wave_reduce(on); });
    // the orientation-free hash (gol/components.hpp) of a 2-D 0/1 array as it stands
    m.def("object_hash", [](py::array_t<u8, py::array::c_style | py::array::forcecast> cells) {
        if (cells.ndim() != 2) throw py::value_error("object_hash: expected a 2-D array");
        return object_hash_host(cells.data(), cells.shape(0), cells.shape(1));
    });

    // ---- match templates (gol/match.hpp) ------------------------------------------------------
    // (what a builder or validate() refuses is a ValueError)
    py::class_<MatchTemplate>(m, "MatchTemplate")
        .def(py::init([](py::array_t<u8, py::array::c_style | py::array::forcecast> value,
                         py::array_t<u8, py::array::c_style | py::array::forcecast> care, i64 ring) {
                 if (value.ndim() != 2 || care.ndim() != 2 || value.shape(0) != care.shape(0) || value.shape(1) != care.shape(1))
                     throw py::value_error("match: value and care must be 2-D arrays of one shape");
                 try {
                     MatchTemplate t = MatchTemplate::from_cells(value.data(), care.data(), value.shape(0), value.shape(1), ring);
                     t.validate();
                     return t;
                 } catch (const Error& e) {
                     throw py::value_error(e.what());
                 }
             }),
             py::arg("value"), py::arg("care"), py::arg("ring") = 0)
        .def_static(
            "from_pattern",
            [](const RlePattern& p, i64 margin) {
                try {
                    MatchTemplate t = MatchTemplate::from_pattern(p, margin);
                    t.validate();
                    return t;
                } catch (const Error& e) {
                    throw py::value_error(e.what());
                }
            },
            py::arg("pattern"), py::arg("margin") = 1)
        .def_readonly("th", &MatchTemplate::th)
        .def_readonly("tw", &MatchTemplate::tw)
        .def_readonly("ring", &MatchTemplate::ring)
        .def_property_readonly("value", [](const MatchTemplate& t) { return template_cells(t, false); })
        .def_property_readonly("care", [](const MatchTemplate& t) { return template_cells(t, true); })
        .def("oriented",
             [](const MatchTemplate& t, int k) {
                 try {
                     return t.oriented(k);
                 } catch (const Error& e) {
                     throw py::value_error(e.what());
                 }
             })
        // [(id, template)]: orientation 0 alone, or all eight without duplicates
        .def("orientations", [](const MatchTemplate& t, bool all) { return t.orientations(all); }, py::arg("all") = true);

    // ---- soup batches ---------------------------------------------------------------------
    // (what the configuration or a call refuses is a ValueError, like a bad rule string)
    py::class_<SoupBatch>(m, "SoupBatch")
        .def(py::init([](i64 n, i64 size, const std::string& rule, const std::string& backend, int device,
                         const std::string& boundary, bool compat, int workgroup) {
                 try {
                     SoupConfig c;
                     c.n = n;
                     c.size = size;
                     c.rule = Rule::parse(rule);
                     c.backend = backend;
                     c.device = device;
                     c.boundary = boundary;
                     c.compat = compat;
                     c.workgroup = workgroup;
                     return SoupBatch::create(c);
                 } catch (const Error& e) {
                     throw py::value_error(e.what());
                 }
             }),
             py::arg("n"), py::arg("size") = 64, py::arg("rule") = "B3/S23", py::arg("backend") = "hip", py::arg("device") = 0,
             py::arg("boundary") = "torus", py::arg("compat") = false, py::arg("workgroup") = 0)
        .def_property_readonly("n", &SoupBatch::n)
        .def_property_readonly("size", &SoupBatch::size)
        .def("init_seed",
             [](SoupBatch& b, u64 seed) {
                 py::gil_scoped_release r;
                 b.init_seed(seed);
             })
        .def("init_boards",
             [](SoupBatch& b, py::array_t<u8, py::array::c_style | py::array::forcecast> cells) {
                 const i64 S = b.size(), M = b.m();
                 if (cells.ndim() != 3 || cells.shape(0) != b.n() || cells.shape(1) != S || cells.shape(2) != S)
                     throw py::value_error(strprintf("soups: the boards are not a (%lld, %lld, %lld) array", (long long)b.n(),
                                                     (long long)S, (long long)S));
                 const u8* p = cells.data();
                 const i64 rows = b.n() * S;
                 std::vector<u64> words((size_t)(rows * M));
                 int bad = -1;
                 {
                     py::gil_scoped_release r;
                     for (i64 row = 0; row < rows && bad < 0; ++row)
                         for (i64 j = 0; j < M; ++j) {
                             u64 v = 0;
                             for (int k = 0; k < 64; ++k) {
                                 const u8 c = p[(size_t)(row * S + 64 * j + k)];
                                 if (c > 1) bad = c;
                                 v |= (u64)(c & 1u) << k;
                             }
                             words[(size_t)(row * M + j)] = v;
                         }
                     if (bad < 0) b.init_words(words.data());
                 }
                 if (bad >= 0) throw py::value_error(strprintf("soups: a board cell is %d, not 0 or 1", bad));
             })
        .def("step",
             [](SoupBatch& b, u64 g) {
                 py::gil_scoped_release r;
                 b.step(g);
             })
        .def(
            "settle",
            [](SoupBatch& b, i64 max_gens, bool transient, i64 chunk) {
                if (max_gens < 0) throw py::value_error(strprintf("soups: max_gens = %lld is negative", (long long)max_gens));
                try {
                    py::gil_scoped_release r;
                    b.settle((u64)max_gens, transient, chunk);
                } catch (const Error& e) {
                    throw py::value_error(e.what());
                }
            },
            py::arg("max_gens"), py::arg("transient") = false, py::arg("chunk") = kSoupDefaultChunk)
        // (period uint32, transient int64, generation uint32, population uint32)
        .def("records",
             [](SoupBatch& b) {
                 std::vector<SoupRecord> rec;
                 {
                     py::gil_scoped_release r;
                     rec = b.records();
                 }
                 const py::ssize_t n = (py::ssize_t)rec.size();
                 py::array_t<u32> period(n), generation(n), population(n);
                 py::array_t<i64> transient(n);
                 for (py::ssize_t i = 0; i < n; ++i) {
                     period.mutable_at(i) = rec[(size_t)i].period;
                     transient.mutable_at(i) = rec[(size_t)i].transient;
                     generation.mutable_at(i) = rec[(size_t)i].generation;
                     population.mutable_at(i) = rec[(size_t)i].population;
                 }
                 return py::make_tuple(period, transient, generation, population);
             })
        .def("boards",
             [](SoupBatch& b, const std::vector<i64>& idx) {
                 std::vector<u8> cells;
                 try {
                     py::gil_scoped_release r;
                     cells = b.boards(idx);
                 } catch (const Error& e) {
                     throw py::value_error(e.what());
                 }
                 py::array_t<u8> a({(py::ssize_t)idx.size(), (py::ssize_t)b.size(), (py::ssize_t)b.size()});
                 std::memcpy(a.mutable_data(), cells.data(), cells.size());
                 return a;
             })
        // dense cells, as the Engine's: (data_ptr, element type code, numel)
        .def("read_boards_cells", [](SoupBatch& b, i64 first, i64 count, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& c) { b.read_boards_cells(first, count, c); }, ptr, code, numel);
        })
        .def("init_cells", [](SoupBatch& b, uintptr_t ptr, int code, i64 numel) {
            cells_call([&](const CellBuffer& c) { b.init_cells(c); }, ptr, code, numel);
        })
        // (n, T) uint32: entry (i, t) the matches of the oriented templates templates[t], summed, on soup i's board
        .def("match_counts",
             [](SoupBatch& b, const std::vector<std::vector<MatchTemplate>>& templates) {
                 std::vector<u32> counts;
                 try {
                     py::gil_scoped_release r;
                     counts = b.match_counts(templates);
                 } catch (const Error& e) {
                     throw py::value_error(e.what());
                 }
                 py::array_t<u32> a({(py::ssize_t)b.n(), (py::ssize_t)templates.size()});
                 if (!counts.empty()) std::memcpy(a.mutable_data(), counts.data(), counts.size() * sizeof(u32));
                 return a;
             })
        // connected components of every soup: components_tuple(), `board` the soup's index
        .def(
            "components",
            [](SoupBatch& b, const std::string& neighbourhood, i64 max_objects, bool hashes, bool records) {
                ComponentsResult res;
                try {
                    const CcNeighbourhood nb = cc_neighbourhood(neighbourhood);
                    py::gil_scoped_release r;
                    res = b.components(nb, max_objects, hashes, records);
                } catch (const Error& e) {
                    throw py::value_error(e.what());
                }
                return components_tuple(res);
            },
            py::arg("neighbourhood") = "moore", py::arg("max_objects") = (i64)1 << 20, py::arg("hashes") = true,
            py::arg("records") = true)
        .def("synchronize",
             [](SoupBatch& b) {
                 py::gil_scoped_release r;
                 b.synchronize();
             })
        .def("stats", [](const SoupBatch& b) {
            const SoupStats s = b.stats();
            py::dict d;
            d["kernel"] = s.kernel;
            d["backend"] = s.backend;
            d["rule"] = s.rule;
            d["launches"] = s.launches;
            d["settled"] = s.settled;
            d["reached"] = s.reached;
            d["workgroup"] = s.workgroup;
            return d;
        });

    // ---- I/O + CLI ------------------------------------------------------------------------
    m.def("dump_filename", &io::dump_filename);
    m.def("dump_header", &io::dump_header);
    m.def("format_rows", [](py::array_t<u64, py::array::c_style | py::array::forcecast> words, i64 w, i64 label0) {
        return py::bytes(io::format_rows(words.data(), words.shape(0), w, words.shape(1), label0));
    });
    m.def("timing_line", &io::timing_line);
    m.attr("BANNER") = std::string(io::kBanner);
    m.attr("USAGE") = std::string(kUsage);
    m.def("run_cli", [](std::vector<std::string> args) {
        std::vector<char*> argv;
        for (auto& s : args) argv.push_back(&s[0]);
        argv.push_back(nullptr);
        py::gil_scoped_release r;
        int rc = run_cli((int)args.size(), argv.data());
        fflush(stdout);
        return rc;
    });

    // ---- devices / bench ------------------------------------------------------------------
    m.def("hip_device_count", []() { return hip_device_count(nullptr); });
    m.def("hip_set_device", &hip_set_device);
    m.def("max_census_depth", []() { return hipk::max_census_depth(); });  // deepest pass of the census kernel
    m.def("max_signature_depth", []() { return hipk::max_signature_depth(); });  // ... of the signature kernel
    m.def("max_film_depth", []() { return hipk::max_film_depth(); });            // ... of the film kernel
    m.def("max_envelope_depth", []() { return hipk::max_envelope_depth(); });    // ... of the envelope kernel
    m.def("max_density_depth", []() { return hipk::max_density_depth(); });      // ... of the density kernel
    // ... of the Generations kernel step_gen for a rule of `states` states (3 .. 9); ValueError on anything else
    m.def("max_generations_depth", [](int states) {
        try {
            return hipk::max_generations_depth(states);
        } catch (const Error& e) {
            throw py::value_error(e.what());
        }
    }, py::arg("states"));
    m.attr("density_film_max_blocks") = kDensityFilmMaxBlocks;                   // blocks of the finest grid density-film mode takes
    m.attr("film_max_cells") = kFilmMaxCells;                                    // cells of the largest window film mode takes
    m.def(
        "naive_byte_run",
        [](i64 N, int gens, int threads, bool sync_each, u64 seed) {
            u64 pop = 0;
            double t;
            {
                py::gil_scoped_release r;
                t = bench::naive_byte_run(N, gens, threads, sync_each, seed, &pop);
            }
            return py::make_tuple(t, pop);
        },
        py::arg("N"), py::arg("gens"), py::arg("threads") = 256, py::arg("sync_each") = true,
        py::arg("seed") = 0x5EED);
    m.def("step_depth_supported", [](int k) { return k >= 1 && k <= 64; });
}
