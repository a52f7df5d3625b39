#=
AlphaGoMI.jl -- thin `ccall` layer that puts libagz.so (MI355X / gfx950) behind the call surface of
tejank10/AlphaGo.jl's self-play hot path, so that `train()` / `selfplay` / the MCTSPlayer tests can
run against it unchanged (SURVEY.md 8b; ABI in include/agz.h).

NOTE: there is no `julia` binary in the build image, so this file has been written against the
Julia manual and the ABI header but never executed.  It contains no arithmetic of its own: every
function is argument marshalling (1-based <-> 0-based, column-major arrays passed as-is) around one
C call.  The Python mirror (alphago.jl_amd/api.py), which IS exercised by the test-suite, has the
same structure call for call.

Index conventions: the reference is 1-based -- flat move f in 1:N^2+1 with f == N^2+1 the pass,
coords (row, col) with row 1 at the top (src/game/go/coords.jl:5-12).  The ABI is 0-based:
a = f - 1, point p = (row-1) + N*(col-1).  Julia arrays are column-major, which is exactly the
layout the ABI documents for boards (N x N Int8), conv weights [kw,kh,cin,cout], dense [out,in],
features N x N x 17 x B and pi A x B -- so arrays cross without copies or permutes.
=#
module AlphaGoMI

using Printf: @sprintf
using Random

export GoEnv, Position, NeuralNet, MCTSPlayer, selfplay, train, extract_data, initialize_game!,
       tree_search!, pick_move, play_move!, should_resign, is_done, set_result!, all_legal_moves,
       score, result, result_string, IllegalMove, to_flat, from_flat, PlayerMove, BLACK, WHITE,
       SelfPlayPlayer, get_replay_batch, Momentum, _train, seed!, analyze, review, reanalyze!, set_starts!, set_playout_cap!, playout_cap_counts, set_forced_playouts!, forced_counts, pruned_pi, set_gumbel!, gumbel_counts, gumbel_pi, set_puct!, puct_counts, set_root_policy_temperature!, set_root_noise!, set_move_temperature!, explore_counts, explore_rows, explore_temperature, extract_targets, value_targets, extract_value_targets, node_lines, most_visited_path, mvp_gg,
       # the node-level surface test/test_mcts.jl:2-5 and test/test_mcts_player.jl:3-6 import
       MCTSNode, select_leaf, maybe_add_child!, add_virtual_loss!, revert_virtual_loss!,
       incorporate_results!, inject_noise!, child_action_score, child_Q, child_U, child_N, child_W,
       child_prior, N, Q, set_N!, suggest_move, get_position, children       # (`position` stays unexported: Base exports a function of that name; node.position and get_position serve)

const libagz = get(ENV, "AGZ_LIB", joinpath(@__DIR__, "..", "libagz.so"))

const BLACK, WHITE, EMPTY = 1, -1, 0

struct IllegalMove <: Exception end          # src/AlphaGo.jl:8

# ---- status codes (include/agz.h)
const AGZ_OK, AGZ_ILLEGAL_MOVE, AGZ_ASSERT_DONE_NODE, AGZ_HISTORY_INCOMPLETE, AGZ_BAD_SHAPE,
      AGZ_ASSERT_SOFTPICK = 0, 1, 2, 3, 4, 5
const AGZ_BAD_ARGUMENT, AGZ_HIP_ERROR, AGZ_POOL_EXHAUSTED, AGZ_RCCL_ERROR, AGZ_NOT_READY = 6, 7, 8, 9, 10

# agz_config: field order and types must match include/agz.h exactly (112 bytes)
struct AgzConfig
  board_size::Int32; tower_height::Int32; games::Int32; num_readouts::Int32
  parallel_readouts::Int32; two_player_mode::Int32
  komi::Float32; reserved0::Float32
  c_puct::Float64; dirichlet_noise_weight::Float64; resign_threshold::Float64
  resign_disable_fraction::Float64
  seed::UInt64; game_id_base::UInt64; game_id_stride::UInt64
  max_nodes_per_game::Int32; device::Int32; external_network::Int32; pool_policy::Int32
  record_capacity_games::Int32; arena_mode::Int32
end

struct AgzPositionInfo
  n::Int32; to_play::Int32; ko::Int32; caps_black::Int32; caps_white::Int32
  last_move::Int32; prev_move::Int32; history_len::Int32; komi::Float32
end

struct AgzNodeInfo
  N::Float32; W::Float32; Q::Float32
  parent::Int32; fmove::Int32; is_expanded::Int32; losses_applied::Int32; done::Int32
  pos::AgzPositionInfo
end

struct AgzGameHeader
  game_id::UInt64; num_moves::Int32; result::Int32; was_resign::Int32; resign_disabled::Int32
  final_score::Float32; short_searches::Int32
end

struct AgzAnalysis         # agz_analysis, include/agz.h: one position's result of analyze
  move::Int32; status::Int32; N::Float32; W::Float32; Q::Float32; nodes_used::Int32
end

struct AgzLine             # agz_line, include/agz.h: one candidate move with its principal variation
  move::Int32; pv_len::Int32; N::Float32; W::Float32; prior::Float32; end_W::Float32
end

struct AgzStats            # agz_stats, include/agz.h: eighteen Int64 counters
  steps::Int64; positions::Int64; games_started::Int64; games_finished::Int64; evals::Int64
  duplicate_evals::Int64; terminal_visits::Int64; root_visits::Int64; nodes_in_use::Int64
  pool_exhausted::Int64; resigned_games::Int64; live_games::Int64; records_dropped::Int64
  pool_short_searches::Int64; peak_nodes_per_game::Int64; stalled_games::Int64; node_capacity::Int64
  abandoned_games::Int64
end

mutable struct Engine
  handle::Ptr{Cvoid}
  cfg::AgzConfig
end

function check(e::Engine, st::Integer)
  st == AGZ_OK && return
  msg = unsafe_string(ccall((:agz_last_error, libagz), Cstring, (Ptr{Cvoid},), e.handle))
  st == AGZ_ILLEGAL_MOVE && throw(IllegalMove())                       # board.jl:265,470
  st in (AGZ_ASSERT_DONE_NODE, AGZ_HISTORY_INCOMPLETE, AGZ_BAD_SHAPE, AGZ_ASSERT_SOFTPICK) &&
    throw(AssertionError(msg))                                          # mcts.jl:190,196 ...
  error("libagz status $st: $msg")
end

function stats(e::Engine)
  st = Ref{AgzStats}()
  check(e, ccall((:agz_engine_stats, libagz), Int32, (Ptr{Cvoid}, Ref{AgzStats}), e.handle, st))
  st[]
end

# a self-play game whose node pool is full plays its move early by default (agz_config.pool_policy, counted in
# stats(e).pool_short_searches and in the game's header); only a game that WAITS on its pool (AGZ_POOL_STALL, or the
# arena, which drops such a game) is an error here
check_pool(e::Engine) = (st = stats(e); (st.stalled_games > 0 || (e.cfg.arena_mode != 0 && st.pool_exhausted > 0)) &&
  error("libagz: a game is waiting on a full node pool (status $AGZ_POOL_EXHAUSTED); raise max_nodes_per_game"))

# agz_slot_status: per slot (status, nodes held, moves played); agz_slot_abandon drops the game in a slot
function slot_status(e::Engine)
  n = Int(e.cfg.games)
  st, nd, mv = zeros(Int32, n), zeros(Int32, n), zeros(Int32, n)
  check(e, ccall((:agz_slot_status, libagz), Int32, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}), e.handle, st, nd, mv))
  st, nd, mv
end
slot_abandon!(e::Engine, slot::Integer) =
  check(e, ccall((:agz_slot_abandon, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, slot))

function Engine(; board_size = 19, tower_height = 19, games = 1, num_readouts = 800,
                parallel_readouts = 8, two_player_mode = false, komi = 7.5, c_puct = 0.96,
                dirichlet_noise_weight = 0.25, resign_threshold = -0.9,
                resign_disable_fraction = 0.05, seed = 0, game_id_base = 0, game_id_stride = 1,
                max_nodes_per_game = 0, device = 0, external_network = false,
                record_capacity_games = 0, arena_mode = false, pool_policy = 0)
  cfg = AgzConfig(board_size, tower_height, games, num_readouts, parallel_readouts,
                  two_player_mode ? 1 : 0, komi, 0f0, c_puct, dirichlet_noise_weight,
                  resign_threshold, resign_disable_fraction, seed, game_id_base, game_id_stride,
                  max_nodes_per_game, device, external_network ? 1 : 0, pool_policy, record_capacity_games,
                  arena_mode ? 1 : 0)
  h = Ref{Ptr{Cvoid}}(C_NULL)
  st = ccall((:agz_engine_create, libagz), Int32, (Ref{AgzConfig}, Ref{Ptr{Cvoid}}), cfg, h)
  st == AGZ_OK || error("agz_engine_create: " *
    unsafe_string(ccall((:agz_last_error, libagz), Cstring, (Ptr{Cvoid},), C_NULL)))
  e = Engine(h[], cfg)
  finalizer(x -> ccall((:agz_engine_destroy, libagz), Cvoid, (Ptr{Cvoid},), x.handle), e)
  e
end

# ------------------------------------------------------------------ GoEnv / Position
# GoEnv(N, planes), src/game/go/go.jl:1-26
struct GoEnv
  N::Int
  action_space::Int
  planes::Int
  max_action_space::Int
  rules::Engine                 # a 1-slot engine used for the batched rule kernels with B = 1
end
GoEnv(board_size::Int = 19, planes::Int = 17) =
  GoEnv(board_size, board_size^2 + 1, (planes - 1) ÷ 2, 361,
        Engine(board_size = board_size, tower_height = 0, games = 1, num_readouts = 1,
               max_nodes_per_game = 8))

to_flat(c, env::GoEnv) = c === nothing ? env.N^2 + 1 : env.N * (c[2] - 1) + c[1]   # coords.jl:6-7
from_flat(f, env::GoEnv) = f == env.N^2 + 1 ? nothing : (1 + (f - 1) % env.N, 1 + (f - 1) ÷ env.N)

struct PlayerMove
  color::Int
  move::Union{Nothing, NTuple{2, Int}}
end

# GoPosition, src/game/go/board.jl:271-306 (the liberty tracker lives on the device side)
mutable struct Position
  env::GoEnv
  board::Matrix{Int8}
  n::Int
  komi::Float32
  caps::NTuple{2, Int}
  ko::Union{Nothing, NTuple{2, Int}}
  recent::Vector{PlayerMove}
  board_deltas::Array{Int8, 3}
  to_play::Int
  done::Bool
end
Position(env::GoEnv; board = zeros(Int8, env.N, env.N), n = 0, komi = 7.5, caps = (0, 0),
         ko = nothing, recent = PlayerMove[], board_deltas = zeros(Int8, env.N, env.N, 0),
         to_play = BLACK) =
  Position(env, board, n, komi, caps, ko, recent, board_deltas, to_play, false)

ko0(pos::Position) = pos.ko === nothing ? Int32(-1) : Int32(to_flat(pos.ko, pos.env) - 1)

# all_legal_moves(pos) -> Vector{Int8}(A), board.jl:393-424
function all_legal_moves(pos::Position)
  e = pos.env.rules
  out = zeros(Int8, pos.env.action_space)
  check(e, ccall((:agz_go_legal, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Int32, Ptr{Int8}),
                 e.handle, pos.board, Int8[pos.to_play], Int32[ko0(pos)], 1, out))
  out
end

# score(pos), board.jl:511-533
function score(pos::Position)
  e = pos.env.rules
  out = zeros(Float32, 1)
  check(e, ccall((:agz_go_score, libagz), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Float32}, Int32, Ptr{Float32}),
                 e.handle, pos.board, Float32[pos.komi], 1, out))
  out[1]
end
result(pos::Position) = (s = score(pos); s > 0 ? 1 : s < 0 ? -1 : 0)          # board.jl:535-544
result_string(s::Real) = s > 0 ? "B+" * @sprintf("%.1f", s) : s < 0 ? "W+" * @sprintf("%.1f", -s) : "DRAW"
result_string(pos::Position) = result_string(score(pos))                      # board.jl:546-555

# play_move!(pos, c; mutate = false), board.jl:451-509 / pass_move! :426-440
function play_move!(pos::Position, c; mutate = false)
  env = pos.env; e = env.rules; N = env.N
  a = to_flat(c, env) - 1
  newboard = similar(pos.board); ko = zeros(Int32, 1); ncap = zeros(Int32, 1); st = zeros(Int32, 1)
  check(e, ccall((:agz_go_play, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int8}, Ptr{Int32},
                  Ptr{Int32}, Ptr{Int32}),
                 e.handle, pos.board, Int8[pos.to_play], Int32[ko0(pos)], Int32[a], 1, newboard, ko, ncap, st))
  st[1] == AGZ_ILLEGAL_MOVE && throw(IllegalMove())
  delta = newboard .- pos.board                       # +color at the move AND where stones vanished?
  # board.jl:479-481: delta[c] = color, delta[captured] = color  (so that prev = new - delta)
  delta = Int8.(ifelse.(delta .!= 0, Int8(pos.to_play), Int8(0)))
  caps = pos.to_play == BLACK ? (pos.caps[1] + ncap[1], pos.caps[2]) : (pos.caps[1], pos.caps[2] + ncap[1])
  keep = min(size(pos.board_deltas, 3), env.planes - 2)
  deltas = cat(dims = 3, reshape(delta, N, N, 1), pos.board_deltas[:, :, 1:keep])
  recent = vcat(pos.recent, PlayerMove(pos.to_play, c))
  done = c === nothing && !isempty(pos.recent) && pos.recent[end].move === nothing
  newko = ko[1] < 0 ? nothing : from_flat(ko[1] + 1, env)
  np = Position(env, newboard, pos.n + 1, pos.komi, caps, newko, recent, deltas, -pos.to_play, done)
  if mutate
    for f in fieldnames(Position); setfield!(pos, f, getfield(np, f)); end
    return pos
  end
  np
end
pass_move!(pos::Position; mutate = false) = play_move!(pos, nothing; mutate = mutate)

# ------------------------------------------------------------------ NeuralNet
# NeuralNet(env; tower_height), src/neural_net.jl:13-33.  Parameters are set layer by layer with
# agz_net_set_weights in Flux layout (conv [kw,kh,cin,cout], dense [out,in]); `load_flux!` walks a
# Flux Chain in `params` order (conv W,b ; BN beta,gamma ; ...), as save_model does (train.jl:14-35).
struct NeuralNet
  env::GoEnv
  tower_height::Int
  engine::Engine
end
function NeuralNet(env::GoEnv; tower_height::Int = 19, seed = 0)
  e = Engine(board_size = env.N, tower_height = tower_height, games = 1, num_readouts = 1,
             max_nodes_per_game = 8)
  check(e, ccall((:agz_net_init_synthetic, libagz), Int32, (Ptr{Cvoid}, UInt64), e.handle, seed))
  NeuralNet(env, tower_height, e)
end

set_weights!(nn::NeuralNet, layer::Integer, kind::Integer, data::AbstractArray{Float32}) =
  check(nn.engine, ccall((:agz_net_set_weights, libagz), Int32,
                         (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Int64),
                         nn.engine.handle, layer, kind, data, length(data)))

# (nn)(positions::Vector{Position}) -> (pi A x B, v 1 x B), src/neural_net.jl:57-68
function (nn::NeuralNet)(positions::Vector{Position})
  env = nn.env; N = env.N; B = length(positions)
  boards = cat(dims = 3, (p.board for p in positions)...)
  deltas = zeros(Int8, N, N, 7, B)
  nd = zeros(Int32, B)
  for (b, p) in enumerate(positions)
    k = size(p.board_deltas, 3); nd[b] = k
    deltas[:, :, 1:k, b] .= p.board_deltas
  end
  tp = Int8[p.to_play for p in positions]
  pi = zeros(Float32, env.action_space, B); v = zeros(Float32, 1, B)
  check(nn.engine, ccall((:agz_net_forward, libagz), Int32,
        (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{Int8}, Int32, Ptr{Float32}, Ptr{Float32}),
        nn.engine.handle, boards, deltas, nd, tp, B, pi, v))
  pi, v
end
(nn::NeuralNet)(pos::Position) = ((p, v) = nn([pos]); (p[:, 1], v[1]))        # neural_net.jl:70-73

# ---- board symmetries (ours; DESIGN.md "Board symmetries").  T_s, s in 0:7, on the 0-based point p = row + N*col:
# s & 4 swaps row and col, then s & 2 flips the row, then s & 1 flips the column.  Engine-wide mode: nothing / -1 (off),
# 0:7 (fixed T_s), :random / 8 (one drawn T_s per network evaluation).
symmetry_mode(s) = s === nothing ? Int32(-1) : s === :random ? Int32(8) : Int32(s)
set_symmetry!(e::Engine, s) =
  check(e, ccall((:agz_selfplay_set_symmetry, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, symmetry_mode(s)))

# feats N x N x 17 x B (or 17N^2 x B): the network on B positions, pi A x B and v B.  symmetry = nothing (the default):
# one orientation, agz_net_forward_features.  An integer s in 0:7, or one per column: column b evaluated under T_s, pi
# back in board orientation (agz_net_forward_features_sym).  :average: the mean pi and v over all eight T_s (each
# position tiled x8 through the _sym entry point, summed in Float64 like the Python mirror).
function forward_features(nn::NeuralNet, feats::Array{Float32}; symmetry = nothing)
  A = nn.env.action_space
  B = length(feats) ÷ (17 * nn.env.N * nn.env.N)
  pi = zeros(Float32, A, B); v = zeros(Float32, B)
  if symmetry === nothing
    check(nn.engine, ccall((:agz_net_forward_features, libagz), Int32,
          (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}, Ptr{Float32}), nn.engine.handle, feats, B, pi, v))
    return pi, v
  end
  if symmetry === :average
    tiled = reshape(repeat(reshape(feats, :, 1, B), 1, 8, 1), :, 8 * B)     # column 8(b-1) + k + 1 = position b, T_k
    p8, v8 = forward_features(nn, tiled; symmetry = repeat(Int32.(0:7), B))
    pm = Float32.(dropdims(sum(Float64.(reshape(p8, A, 8, B)), dims = 2), dims = 2) ./ 8)
    vm = Float32.(vec(sum(Float64.(reshape(v8, 8, B)), dims = 1)) ./ 8)
    return pm, vm
  end
  sym = symmetry isa Integer ? fill(Int32(symmetry), B) : Int32.(collect(symmetry))
  @assert length(sym) == B
  check(nn.engine, ccall((:agz_net_forward_features_sym, libagz), Int32,
        (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Float32}),
        nn.engine.handle, feats, sym, B, pi, v))
  pi, v
end

# ------------------------------------------------------------------ MCTSPlayer (single tree, slot 0)
# MCTSPlayer(env, network; num_readouts, two_player_mode, resign_threshold), mcts_play.jl:3-24.
# `network` is any callable positions -> (pi, v) (duck-typed field, mcts_play.jl:5): a NeuralNet of
# this module is evaluated on the device without leaving it; anything else (DummyNet, a Flux model)
# receives the leaves' feature tensor through the select / incorporate split.
mutable struct MCTSPlayer
  env::GoEnv
  network
  num_readouts::Int
  two_player_mode::Bool
  τ_threshold::Int
  qs::Vector{Float32}
  searches_π::Vector{Vector{Float32}}
  result::Int
  result_string::String
  resign_threshold::Float64
  engine::Engine
  start::Union{Nothing, Position}       # the position initialize_game! was given
  recent::Vector{PlayerMove}            # start.recent + every move played since: root.position.recent (board.jl:299)
end
function MCTSPlayer(env::GoEnv, network; num_readouts = 800, two_player_mode = false,
                    resign_threshold = -0.9, seed = 0, symmetry = nothing, fpu = nothing, c_base::Real = 0.0,
                    root_policy_temperature = nothing, root_noise = nothing, move_temperature = nothing)
  τ = two_player_mode ? -1 : (env.N * env.N ÷ 12) ÷ 2 * 2
  th = network isa NeuralNet ? network.tower_height : 0
  e = Engine(board_size = env.N, tower_height = th, games = 1, num_readouts = num_readouts,
             parallel_readouts = 64, two_player_mode = two_player_mode,
             resign_threshold = resign_threshold, seed = seed, external_network = !(network isa NeuralNet))
  symmetry === nothing || set_symmetry!(e, symmetry)
  apply_puct!(e, fpu, c_base)
  apply_explore!(e, root_policy_temperature, root_noise, move_temperature)
  MCTSPlayer(env, network, num_readouts, two_player_mode, τ, Float32[], Vector{Float32}[], 0, "",
             resign_threshold, e, nothing, PlayerMove[])
end

# A Position in the C ABI's terms (agz_tree_init, agz_analyze_start): board, AgzPositionInfo and the older boards.
# The reference keeps pos.board_deltas (board.jl:505-506); the engine wants the older boards themselves, newest first:
# B_{k+1} = B_k - delta_k (features.jl:8-14)
function position_arrays(env::GoEnv, pos::Position)
  last = isempty(pos.recent) ? -1 : to_flat(pos.recent[end].move, env) - 1
  k = min(7, size(pos.board_deltas, 3))
  hist = Matrix{Int8}(undef, length(pos.board), k)
  b = copy(pos.board)
  for i in 1:k
    b = b .- pos.board_deltas[:, :, i]
    hist[:, i] = vec(b)
  end
  prev = length(pos.recent) < 2 ? -1 : to_flat(pos.recent[end-1].move, env) - 1
  info = AgzPositionInfo(pos.n, pos.to_play, ko0(pos), pos.caps[1], pos.caps[2], last, prev, k, pos.komi)
  pos.board, info, hist
end

function initialize_game!(p::MCTSPlayer, pos = nothing)                        # mcts_play.jl:110-118
  pos === nothing && (pos = Position(p.env))
  _, info, hist = position_arrays(p.env, pos)
  k = Int(info.history_len)
  check(p.engine, ccall((:agz_tree_init, libagz), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int8}, Ref{AgzPositionInfo}, Ptr{Int8}),
        p.engine.handle, 0, pos.board, info, k == 0 ? C_NULL : hist))      # ccall roots `hist` for the call
  p.result = 0; p.qs = Float32[]; p.searches_π = Vector{Float32}[]
  p.start = pos; p.recent = copy(pos.recent)
  p
end

function root(p::MCTSPlayer)
  r = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_root, libagz), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}), p.engine.handle, 0, r))
  r[]
end

function node_info(p::MCTSPlayer, node)
  info = Ref{AgzNodeInfo}()
  check(p.engine, ccall((:agz_tree_node_info, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{AgzNodeInfo}),
                        p.engine.handle, 0, node, info))
  info[]
end
N(p::MCTSPlayer) = node_info(p, root(p)).N
Q(p::MCTSPlayer) = node_info(p, root(p)).Q

function child_N(p::MCTSPlayer)
  out = zeros(Float32, p.env.action_space)
  check(p.engine, ccall((:agz_tree_node_floats, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float32}),
                        p.engine.handle, 0, root(p), 0, out))
  out
end

# The leaves the last agz_tree_search_select collected, as the reference's GoPosition fields (agz_tree_leaf_positions):
# node handles and, unless `nodes_only`, one Position per leaf -- board, board_deltas (newest first), to_play, n, ko,
# caps, the last two moves.
function leaf_positions(p::MCTSPlayer, B::Int; nodes_only::Bool = false)
  env = p.env; N = env.N
  nodes = zeros(Int32, B)
  if nodes_only
    check(p.engine, ccall((:agz_tree_leaf_positions, libagz), Int32,
          (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{Int8}, Ptr{AgzPositionInfo}),
          p.engine.handle, 0, nodes, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    return nodes, Position[]
  end
  boards = zeros(Int8, N, N, B); deltas = zeros(Int8, N, N, 7, B); nd = zeros(Int32, B); tp = zeros(Int8, B)
  info = Vector{AgzPositionInfo}(undef, B)
  check(p.engine, ccall((:agz_tree_leaf_positions, libagz), Int32,
        (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{Int8}, Ptr{AgzPositionInfo}),
        p.engine.handle, 0, nodes, boards, deltas, nd, tp, info))
  to_pm(a, color) = PlayerMove(color, a == N^2 ? nothing : from_flat(a + 1, env))
  positions = Position[]
  for b in 1:B
    i = info[b]
    recent = PlayerMove[]
    i.prev_move >= 0 && push!(recent, to_pm(Int(i.prev_move), Int(i.to_play)))
    i.last_move >= 0 && push!(recent, to_pm(Int(i.last_move), -Int(i.to_play)))
    push!(positions, Position(env, boards[:, :, b], Int(i.n), i.komi, (Int(i.caps_black), Int(i.caps_white)),
                              i.ko < 0 ? nothing : from_flat(i.ko + 1, env), recent,
                              deltas[:, :, 1:nd[b], b], Int(i.to_play), false))
  end
  nodes, positions
end

# Tracker-era networks answer with TrackedArrays (the reference's DummyNet returns `param(...)`,
# test/test_mcts_player.jl:22-32); mcts_play.jl:90 unwraps them with `.data`
untrack(x) = hasproperty(x, :data) ? getproperty(x, :data) : x

# tree_search!(player, parallel_readouts = 8), mcts_play.jl:73-98; returns the leaves (Vector{MCTSNode}) like the
# reference.  A caller-supplied network receives `positions::Vector{Position}` with length(positions) == number of
# leaves -- the reference's `mcts_player.network([leaf.position for leaf in leaves])` (mcts_play.jl:89).
function tree_search!(p::MCTSPlayer, parallel_readouts = 8)
  n = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_search_select, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}),
                        p.engine.handle, 0, parallel_readouts, n))
  B = Int(n[])
  if p.network isa NeuralNet || B == 0              # the engine's own network evaluates the leaves on the device
    nodes, _ = B == 0 ? (Int32[], Position[]) : leaf_positions(p, B; nodes_only = true)
    check(p.engine, ccall((:agz_tree_search_incorporate, libagz), Int32,
                          (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}), p.engine.handle, 0, C_NULL, C_NULL))
    return [MCTSNode(p, id) for id in nodes]
  end
  nodes, positions = leaf_positions(p, B)
  move_probs, values = p.network(positions)                                     # mcts_play.jl:89
  move_probs, values = untrack(move_probs), untrack(values)                     # :90
  size(move_probs) == (p.env.action_space, B) && length(values) == B ||
    throw(AssertionError("network returned $(size(move_probs)) / $(length(values)) values for $B positions"))
  check(p.engine, ccall((:agz_tree_search_incorporate, libagz), Int32,
                        (Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}),
                        p.engine.handle, 0, Matrix{Float32}(move_probs), Vector{Float32}(vec(values))))
  [MCTSNode(p, id) for id in nodes]
end

function pick_move(p::MCTSPlayer)                                               # mcts_play.jl:52-71
  a = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_pick_move, libagz), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}), p.engine.handle, 0, a))
  from_flat(a[] + 1, p.env)
end

function play_move!(p::MCTSPlayer, c)                                           # mcts_play.jl:26-50
  info = node_info(p, root(p))
  π = child_N(p)
  if !p.two_player_mode
    # children_as_pi(root, n <= tau) (mcts.jl:241-252): the device records the same vector in its
    # game record; the host copy here serves `searches_π` for callers that read the field directly
    squash = info.pos.n <= p.τ_threshold
    pr = squash ? Float64.(π) .^ 0.98 : π
    push!(p.searches_π, Float32.(pr ./ sum(pr)))
  end
  push!(p.qs, info.Q)
  ok = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_play_move, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}),
                        p.engine.handle, 0, to_flat(c, p.env) - 1, ok))
  if ok[] == 0
    println("Illegal move")
    !p.two_player_mode && pop!(p.searches_π)
    pop!(p.qs)
    return false
  end
  push!(p.recent, PlayerMove(Int(info.pos.to_play), c))
  true
end

# ------------------------------------------------------------------ MCTSNode (node-level surface)
# The reference's tests drive single nodes (test/test_mcts.jl:2-5, test/test_mcts_player.jl:3-6): an MCTSNode here is
# a handle -- the player whose tree it lives in and the slot-local node id of include/agz.h -- and every function
# below is one agz_tree_* call.  `player.root` reads as in the reference (a property, below).
struct MCTSNode
  player::MCTSPlayer
  id::Int32
end
Base.getproperty(p::MCTSPlayer, s::Symbol) =
  s === :root ? MCTSNode(p, root(p)) : s === :position ? position(MCTSNode(p, root(p))) : getfield(p, s)
Base.:(==)(a::MCTSNode, b::MCTSNode) = getfield(a, :player) === getfield(b, :player) && getfield(a, :id) == getfield(b, :id)
# The reference's tests read a node's state as FIELDS (test/test_mcts.jl:52-70, test/test_mcts_player.jl:150-175:
# node.position, .children, .child_N, .child_prior, .fmove, .parent, .is_expanded ...; src/mcts.jl:41-53): each is one
# accessor call on the device tree (ADVICE r4).  `fmove` is 1-based as in the reference (nothing for a root); `parent`
# is an MCTSNode (nothing for a root: the reference's DummyNode carries no state a test reads).
function Base.getproperty(x::MCTSNode, s::Symbol)
  (s === :player || s === :id) && return getfield(x, s)
  s === :position && return position(x)
  s === :children && return children(x)
  s === :child_N && return child_N(x)
  s === :child_W && return child_W(x)
  s === :child_prior && return child_prior(x)
  s === :original_prior && return child_prior(x)      # mcts.jl:49: equal until inject_noise! (the device keeps one row)
  info = node_info(x)
  s === :fmove && return info.fmove < 0 ? nothing : Int(info.fmove) + 1
  s === :parent && return info.parent < 0 ? nothing : MCTSNode(getfield(x, :player), info.parent)
  s === :is_expanded && return info.is_expanded != 0
  s === :losses_applied && return Int(info.losses_applied)
  error("MCTSNode has no field $s")
end
Base.propertynames(::MCTSNode) = (:player, :id, :position, :children, :child_N, :child_W, :child_prior, :original_prior,
                                  :fmove, :parent, :is_expanded, :losses_applied)

node_info(x::MCTSNode) = node_info(x.player, x.id)
N(x::MCTSNode) = node_info(x).N                                                 # mcts.jl:98-100
Q(x::MCTSNode) = node_info(x).Q                                                 # mcts.jl:94
function node_floats(x::MCTSNode, field::Integer)
  e = x.player.engine
  out = zeros(Float32, x.player.env.action_space)
  check(e, ccall((:agz_tree_node_floats, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float32}),
                 e.handle, 0, x.id, field, out))
  out
end
child_N(x::MCTSNode) = node_floats(x, 0)
child_W(x::MCTSNode) = node_floats(x, 1)
child_prior(x::MCTSNode) = node_floats(x, 2)
child_Q(x::MCTSNode) = child_W(x) ./ (1 .+ child_N(x))                          # mcts.jl:89
# mcts.jl:91-92, in the reference's own mixed precision (c_puct is Float64, the square root is Float32's)
child_U(x::MCTSNode) = (x.player.engine.cfg.c_puct * √(1 .+ N(x)) * child_prior(x) ./ (1 .+ child_N(x)))
function child_action_score(x::MCTSNode)                                         # mcts.jl:86-87 (Float64 scores)
  e = x.player.engine
  out = zeros(Float64, x.player.env.action_space)
  check(e, ccall((:agz_tree_node_scores, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float64}),
                 e.handle, 0, x.id, out))
  out
end
function set_N!(x::MCTSNode, value)                                             # mcts.jl:99
  e = x.player.engine
  check(e, ccall((:agz_tree_node_set_N, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Float32),
                 e.handle, 0, x.id, Float32(value)))
  value
end

function select_leaf(x::MCTSNode)                                               # mcts.jl:108-138
  e = x.player.engine
  leaf = Ref{Int32}(0)
  check(e, ccall((:agz_tree_select_leaf, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}),
                 e.handle, 0, x.id, leaf))
  MCTSNode(x.player, leaf[])
end
function maybe_add_child!(x::MCTSNode, f::Integer)                              # mcts.jl:140-149; f is 1-based
  e = x.player.engine
  child = Ref{Int32}(0)
  check(e, ccall((:agz_tree_maybe_add_child, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32, Ref{Int32}),
                 e.handle, 0, x.id, f - 1, child))
  MCTSNode(x.player, child[])
end
# `up_to` is the node the walk towards the root stops at (mcts.jl:151-177); the tests pass `player.root`
function add_virtual_loss!(x::MCTSNode, up_to::MCTSNode)
  e = x.player.engine
  check(e, ccall((:agz_tree_add_virtual_loss, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32),
                 e.handle, 0, x.id, up_to.id))
end
function revert_virtual_loss!(x::MCTSNode, up_to::MCTSNode)
  e = x.player.engine
  check(e, ccall((:agz_tree_revert_virtual_loss, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32),
                 e.handle, 0, x.id, up_to.id))
end
function incorporate_results!(x::MCTSNode, move_probs, value, up_to::MCTSNode)  # mcts.jl:187-214
  e = x.player.engine
  probs = Float32.(vec(move_probs))
  check(e, ccall((:agz_tree_incorporate, libagz), Int32,
                 (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Int32, Float32, Int32),
                 e.handle, 0, x.id, probs, length(probs), Float32(value), up_to.id))
end
function inject_noise!(x::MCTSNode)                                             # mcts.jl:232-239
  e = x.player.engine
  check(e, ccall((:agz_tree_inject_noise, libagz), Int32, (Ptr{Cvoid}, Int32, Int32), e.handle, 0, x.id))
end
function is_done(x::MCTSNode)                                                   # mcts.jl:227-229
  e = x.player.engine
  r = Ref{Int32}(0)
  check(e, ccall((:agz_tree_is_done, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}), e.handle, 0, x.id, r))
  r[] != 0
end
function children(x::MCTSNode)                                                  # Dict(flat move => child), mcts.jl:51
  e = x.player.engine
  ids = zeros(Int32, x.player.env.action_space)
  check(e, ccall((:agz_tree_node_children, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}),
                 e.handle, 0, x.id, ids))
  Dict(f => MCTSNode(x.player, ids[f]) for f in eachindex(ids) if ids[f] >= 0)
end
# ---- analysis lines (ours; most_visited_path / mvp_gg / describe of mcts.jl:255-327, commented out there, are the
# definition: include/agz.h "analysis lines").  A line is a NamedTuple: move and pv as board coordinates (nothing = pass,
# pv[1] == move), N / W / prior = the candidate's entries of the node's rows, Q = W / (1 + N), pv_N[d] = the child_N entry
# pv[d] was chosen by, end_Q = Q of the line's last move.
kgs_name(c, env::GoEnv) = c === nothing ? "pass" : string("ABCDEFGHJKLMNOPQRST"[c[2]], env.N + 1 - c[1])
function line_rows(env::GoEnv, ln::AbstractVector{AgzLine}, pv::AbstractMatrix{Int16}, pvn::AbstractMatrix{Float32})
  out = NamedTuple[]
  for k in eachindex(ln)
    l = ln[k]
    (l.move < 0 || l.pv_len < 1) && continue
    n = Int(l.pv_len)
    push!(out, (move = from_flat(l.move + 1, env), N = l.N, W = l.W, Q = l.W / (1f0 + l.N), prior = l.prior,
                pv = [from_flat(Int(a) + 1, env) for a in pv[1:n, k]], pv_N = pvn[1:n, k],
                end_Q = l.end_W / (1f0 + pvn[n, k])))
  end
  out
end
# the top k candidates of node x (child_N, then child_prior descending, then the move ascending) with their principal
# variations of at most `depth` moves: one agz_tree_lines call, the walk runs on the device
function node_lines(x::MCTSNode, k::Integer = 4, depth::Integer = 16, min_visits::Integer = 1)
  e = x.player.engine
  ln = Vector{AgzLine}(undef, k); pv = zeros(Int16, depth, k); pvn = zeros(Float32, depth, k)
  check(e, ccall((:agz_tree_lines, libagz), Int32,
                 (Ptr{Cvoid}, Int32, Int32, Int32, Int32, Int32, Ptr{AgzLine}, Ptr{Int16}, Ptr{Float32}),
                 e.handle, 0, x.id, k, depth, min_visits, ln, pv, pvn))
  line_rows(x.player.env, ln, pv, pvn)
end
function most_visited_path(x::MCTSNode)                                         # mcts.jl:267-281
  ln = node_lines(x, 1, 64, 1)
  isempty(ln) && return @sprintf("Q: %.5f\n", Q(x))
  env = x.player.env
  join(["$(kgs_name(c, env)) ($(n)) ==> " for (c, n) in zip(ln[1].pv, ln[1].pv_N)]) * @sprintf("Q: %.5f\n", ln[1].end_Q)
end
function mvp_gg(x::MCTSNode)                                                    # mcts.jl:283-293
  ln = node_lines(x, 1, 64, 2)
  (isempty(ln) || !(ln[1].N > 1)) && return ""
  join([kgs_name(c, x.player.env) for c in ln[1].pv], " ")
end

function position(x::MCTSNode)                                                  # the node's GoPosition, mcts.jl:44
  p = x.player; e = p.engine; env = p.env
  info = node_info(x)
  board = zeros(Int8, env.N, env.N)
  check(e, ccall((:agz_tree_node_board, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Int8}),
                 e.handle, 0, x.id, board))
  pos = Position(env)
  pos.board = board; pos.n = info.pos.n; pos.komi = info.pos.komi
  pos.caps = (Int(info.pos.caps_black), Int(info.pos.caps_white))
  pos.ko = info.pos.ko < 0 ? nothing : from_flat(info.pos.ko + 1, env)
  pos.to_play = info.pos.to_play
  pos.done = info.done != 0
  # `recent`: the C ABI exposes the last two moves of a node (agz_position_info.last_move / prev_move: what select_leaf's
  # pass rule and the double-pass end need, mcts.jl:119-126); the full move list of a game is extract_data's
  # (agz_records_game).  `board_deltas` is not rebuilt here: features come from agz_features / the leaf feature call.
  to_pm(a, color) = PlayerMove(color, a == env.N^2 ? nothing : from_flat(a + 1, env))
  if x.id == root(p)
    pos.recent = copy(getfield(p, :recent))       # the player's root: the game's whole move list (extract_data replays it)
  else
    if info.pos.prev_move >= 0 push!(pos.recent, to_pm(Int(info.pos.prev_move), pos.to_play)) end
    if info.pos.last_move >= 0 push!(pos.recent, to_pm(Int(info.pos.last_move), -pos.to_play)) end
  end
  pos
end

get_position(p::MCTSPlayer) = position(p.root)                                  # mcts_play.jl:141-142

function suggest_move(p::MCTSPlayer)                                            # mcts_play.jl:144-151
  current_readouts = N(p)
  while N(p) < current_readouts + p.num_readouts
    tree_search!(p)
  end
  pick_move(p)
end

function should_resign(p::MCTSPlayer)                                           # mcts_play.jl:124
  r = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_should_resign, libagz), Int32, (Ptr{Cvoid}, Int32, Ref{Int32}), p.engine.handle, 0, r))
  r[] != 0
end

function is_done(p::MCTSPlayer)                                                 # mcts_play.jl:120
  p.result != 0 && return true
  r = Ref{Int32}(0)
  check(p.engine, ccall((:agz_tree_is_done, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Int32}),
                        p.engine.handle, 0, root(p), r))
  r[] != 0
end

function set_result!(p::MCTSPlayer, winner, was_resign)                         # mcts_play.jl:100-108
  p.result = winner
  p.result_string = was_resign ? (winner == BLACK ? "B+R" : "W+R") : result_string(position(p.root))
end

# replay_position(pos, result), board.jl:557-578: the positions before each move of `recent`, from the empty board
function replay_positions(env::GoEnv, komi, recent::Vector{PlayerMove})
  positions = Position[]
  pos = Position(env; komi = komi)
  for pm in recent
    push!(positions, pos)
    pos = play_move!(pos, pm.move)
  end
  positions, pos
end

# extract_data(player) -> (positions, pis, results), mcts_play.jl:126-139 -- ONE argument, as train.jl:58 calls it
function extract_data(p::MCTSPlayer)
  rootpos = position(p.root)
  length(p.searches_π) == rootpos.n || throw(AssertionError("length(searches_π) == root.position.n"))      # :127
  rootpos.n == length(rootpos.recent) || throw(AssertionError("GoPosition history is incomplete"))          # board.jl:568
  positions, _ = replay_positions(p.env, rootpos.komi, rootpos.recent)
  positions, deepcopy(p.searches_π), fill(p.result, length(positions))
end

# ------------------------------------------------------------------ self-play
# selfplay(env, nn, num_ro) -> the finished game's player (src/selfplay.jl:1-45,:44), exactly the call train() makes
# (train.jl:57).  With `games = G` (ours) the same loop runs for G concurrent games on the device and a Vector of the
# same objects comes back, ordered by game id.
#
# SelfPlayPlayer is the MCTSPlayer of ONE finished game, read-only: the fields train() and extract_data read
# (mcts_play.jl:3-15) -- result, result_string, qs, searches_π, root.position (the final GoPosition with its whole
# `recent`: .n, .board, .caps ...) -- as the device recorded them.  The tree stayed on the device and its slot was
# recycled.  It also carries the record's own fields (game_id, moves as 1-based flat moves, short_searches).
struct FinishedRoot
  position::Position
end
struct SelfPlayPlayer
  env::GoEnv
  network
  num_readouts::Int
  two_player_mode::Bool
  τ_threshold::Int
  qs::Vector{Float32}
  searches_π::Vector{Vector{Float32}}
  result::Int
  result_string::String
  root::FinishedRoot
  resign_threshold::Float64
  position::Position
  positions::Vector{Position}           # the position before each move (replay_position, board.jl:557-578)
  game_id::UInt64
  moves::Vector{Int}                    # 1-based flat moves, N^2+1 = pass
  short_searches::Int                   # moves played on fewer than num_ro readouts (full node pool, agz_config.pool_policy); 0 = the reference's game
  start::Union{Nothing, Position}       # the position the game began at (selfplay(...; starts)), nothing = the empty board
  start_index::Int                      # its 0-based entry of the table of start positions, -1 = none
  full_search::Vector{Bool}             # per move: false for a fast search of selfplay(...; playout_cap), whose searches_π entry is all zero
end
is_done(p::SelfPlayPlayer) = true
get_position(p::SelfPlayPlayer) = p.root.position

# extract_data(player), mcts_play.jl:126-139: every result entry is the final game result
function extract_data(p::SelfPlayPlayer)
  n0 = p.start === nothing ? 0 : p.start.n
  length(p.searches_π) == p.root.position.n - n0 || throw(AssertionError("length(searches_π) == root.position.n - start.n"))
  copy(p.positions), deepcopy(p.searches_π), fill(p.result, length(p.positions))
end

# extract_data without the plies of fast searches (selfplay(...; playout_cap)): their all-zero π rows are no policy targets
function extract_targets(p::SelfPlayPlayer)
  positions, pis, results = extract_data(p)
  keep = findall(p.full_search)
  positions[keep], pis[keep], results[keep]
end

# The reference draws from Julia's global RNG (selfplay.jl:9, mcts.jl:133,235, mcts_play.jl:61,66), so successive
# selfplay calls see successive random numbers.  The engine's draws are a function of (seed, game id, move, site)
# (include/agz_draws.h): seed!(s) is Random.seed!(s) for it, and every selfplay call plays the next unused game ids.
const STREAM = Ref((UInt64(0), UInt64(0)))                     # (seed, next game id)
seed!(s::Integer) = (STREAM[] = (UInt64(s), UInt64(0)); nothing)

# A table of start positions (ours; include/agz.h agz_selfplay_set_starts): the self-play game with id gid begins at
# starts[gid % S + 1] -- initialize_game!(player, pos), mcts_play.jl:110-118 -- and arena game g at starts[g % S + 1];
# everything that replays the records begins there too.  An empty vector clears the table.
function set_starts!(e::Engine, env::GoEnv, starts::Vector{Position})
  S, P = length(starts), env.N * env.N
  boards = zeros(Int8, P, max(S, 1)); hist = zeros(Int8, P, 7, max(S, 1)); info = Vector{AgzPositionInfo}(undef, max(S, 1))
  for (i, pos) in enumerate(starts)
    b, info[i], h = position_arrays(env, pos)
    boards[:, i] = vec(b); hist[:, 1:size(h, 2), i] = h
  end
  check(e, ccall((:agz_selfplay_set_starts, libagz), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{AgzPositionInfo}, Ptr{Int8}, Int64),
                 e.handle, boards, info, hist, S))
end
starts_count(e::Engine) = Int(ccall((:agz_selfplay_starts_count, libagz), Int64, (Ptr{Cvoid},), e.handle))

# Playout cap randomization (ours; include/agz.h agz_selfplay_set_playout_cap): the search of the root of ply n is full
# (noise, num_readouts, π recorded) iff u01(draw(seed, game, n, site 11, 0)) < p, else fast (no noise, r readouts, the
# ply's π row all zero: no policy target).  r = 0 switches it off.
function set_playout_cap!(e::Engine, r::Integer, p::Real)
  check(e, ccall((:agz_selfplay_set_playout_cap, libagz), Int32, (Ptr{Cvoid}, Int32, Float64), e.handle, r, p))
end
# (full, fast) moves played since agz_selfplay_start while the cap was on
function playout_cap_counts(e::Engine)
  out = zeros(Int64, 2)
  check(e, ccall((:agz_selfplay_playout_cap_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{Int64}), e.handle, out))
  Int(out[1]), Int(out[2])
end
# the arena's entries are the plies with a non-zero π row (agz_replay_set_targets_only); only while it is empty
function replay_set_targets_only!(e::Engine, on::Bool = true)
  check(e, ccall((:agz_replay_set_targets_only, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, on ? 1 : 0))
end

# Search-value targets (ours; include/agz.h agz_replay_set_value_target, include/agz_value_target.h): the z of the arena's
# batch calls becomes y_t = (1 - alpha) * result + alpha * G_t, G_t the TD(lam) return of the record's qs from ply t on
# (backward Horner in Float64, every product and sum rounded on its own).  alpha = 0 (the default) is off.
function replay_set_value_target!(e::Engine, alpha::Real = 0.0, lam::Real = 1.0)
  check(e, ccall((:agz_replay_set_value_target, libagz), Int32, (Ptr{Cvoid}, Float64, Float64), e.handle, alpha, lam))
end
# y [num_moves] of ring record k (0-based, agz_records_game's numbering)
function records_value_targets(e::Engine, k::Integer, alpha::Real, lam::Real)
  h = Ref{AgzGameHeader}()
  check(e, ccall((:agz_records_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
  out = zeros(Float32, max(Int(h[].num_moves), 1))
  check(e, ccall((:agz_records_value_targets, libagz), Int32, (Ptr{Cvoid}, Int64, Float64, Float64, Ptr{Float32}),
                 e.handle, k, alpha, lam, out))
  out[1:h[].num_moves]
end
# the same for a record held on the host (no engine): qs the recorded root values, result the outcome
function value_targets(qs::Vector{Float32}, result::Integer, alpha::Real, lam::Real)
  out = zeros(Float32, length(qs))
  st = ccall((:agz_value_targets, libagz), Int32, (Ptr{Float32}, Int32, Int32, Float64, Float64, Ptr{Float32}),
             qs, length(qs), result, alpha, lam, out)
  st == 0 || throw(ArgumentError("value targets: alpha $alpha and lam $lam must both lie in 0..1"))
  out
end
# extract_data with the per-ply value targets as `results` instead of the constant fill; value_target = (alpha, lam).
# (extract_data itself keeps the reference's one-argument form, as extract_targets does for the playout cap.)
function extract_value_targets(p::Union{MCTSPlayer, SelfPlayPlayer}, value_target; targets_only::Bool = false)
  positions, pis, _ = extract_data(p)
  y = value_targets(Vector{Float32}(p.qs), p.result, value_target[1], value_target[2])
  keep = (targets_only && p isa SelfPlayPlayer) ? findall(p.full_search) : collect(1:length(positions))
  positions[keep], pis[keep], y[keep]        # a kept ply sums the qs of the dropped plies behind it
end

# Policy surprise weighting (ours; include/agz.h agz_replay_score, include/agz_surprise.h): one KL(π ‖ prior) per ply of
# arena games first .. first+count-1 (0-based) on the selected network; under rho > 0 agz_replay_sample draws by weight,
# with replacement -- per scored game a share 1 - rho of the mass evenly over its target plies, rho in proportion to the
# scores.  rho = 0 (the default) is off.
function replay_score!(e::Engine, first::Integer = 0, count::Union{Nothing, Integer} = nothing)
  n = count === nothing ? ccall((:agz_replay_count, libagz), Int64, (Ptr{Cvoid},), e.handle) - first : count
  rows = Ref{Int64}(0)
  check(e, ccall((:agz_replay_score, libagz), Int32, (Ptr{Cvoid}, Int64, Int64, Ref{Int64}), e.handle, first, n, rows))
  Int(rows[])
end
function replay_set_surprise!(e::Engine, rho::Real = 0.0)
  check(e, ccall((:agz_replay_set_surprise, libagz), Int32, (Ptr{Cvoid}, Float64), e.handle, rho))
end
# (kl [num_moves], q [num_moves] under the rho in force, scored) of arena game k (0-based)
function replay_surprise(e::Engine, k::Integer)
  h = Ref{AgzGameHeader}()
  check(e, ccall((:agz_replay_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
  n = Int(h[].num_moves)
  kl, q, sc = zeros(Float64, max(n, 1)), zeros(UInt32, max(n, 1)), Ref{Int32}(0)
  check(e, ccall((:agz_replay_surprise, libagz), Int32, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{UInt32}, Ref{Int32}),
                 e.handle, k, kl, q, sc))
  kl[1:n], q[1:n], sc[] != 0
end
# the same for one game held on the host (no engine): pis and ps are A x T (one column per ply, as the C rows lie)
function surprise_weights(pis::Matrix{Float32}, ps::Matrix{Float32}, rho::Real)
  A, T = size(pis)
  size(ps) == (A, T) || throw(ArgumentError("surprise weights: pis and ps must have the same size"))
  kl, q = zeros(Float64, T), zeros(UInt32, T)
  st = ccall((:agz_surprise_weights, libagz), Int32,
             (Ptr{Float32}, Ptr{Float32}, Int32, Int32, Float64, Ptr{Float64}, Ptr{UInt32}), pis, ps, T, A, rho, kl, q)
  st == 0 || throw(ArgumentError("surprise weights: rho $rho must lie in 0..1"))
  kl, q
end
# the index agz_replay_sample's weighted draw picks for the 64-bit draw u in the inclusive prefix cum (0-based; -1: no mass)
surprise_pick(cum::Vector{UInt64}, u::UInt64) =
  Int(ccall((:agz_surprise_pick, libagz), Int64, (Ptr{UInt64}, Int64, UInt64), cum, length(cum), u))

# Forced playouts and policy target pruning (ours; include/agz.h agz_selfplay_set_forced_playouts): in a full self-play
# search a visited root child a with N_a^2 < k P_a sum(N) is selected ahead of the PUCT arg-max; with prune the recorded π
# row leaves out the forced visits the search did not agree with.  k = 0 switches both off; KataGo plays k = 2.
function set_forced_playouts!(e::Engine, k::Real, prune::Bool = true)
  check(e, ccall((:agz_selfplay_set_forced_playouts, libagz), Int32, (Ptr{Cvoid}, Float64, Int32), e.handle, k,
                 (prune && k != 0) ? 1 : 0))
end
# (root descents the forced rule decided, recorded π rows that pruning changed) since agz_selfplay_start
function forced_counts(e::Engine)
  out = zeros(Int64, 2)
  check(e, ccall((:agz_selfplay_forced_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{Int64}), e.handle, out))
  Int(out[1]), Int(out[2])
end
# the pruned π row of node `node` of single tree g under k, whatever the engine's setting
function pruned_pi(e::Engine, g::Integer, node::Integer, k::Real, A::Integer)
  out = zeros(Float32, A)
  check(e, ccall((:agz_tree_pruned_pi, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Float32}), e.handle, g,
                 node, k, out))
  out
end

# Gumbel root search (ours; include/agz.h agz_selfplay_set_gumbel): a full self-play search samples up to m root
# candidates by Gumbel-top-k, spends its readouts on them by Sequential Halving, plays the survivor with the largest
# g + logit + σ(q) and records softmax(logit + σ(q)) as the π row.  m = 0 switches it off; not together with forced playouts.
function set_gumbel!(e::Engine, m::Integer, c_visit::Real = 50.0, c_scale::Real = 1.0)
  check(e, ccall((:agz_selfplay_set_gumbel, libagz), Int32, (Ptr{Cvoid}, Int32, Float64, Float64), e.handle, m, c_visit,
                 c_scale))
end
# (Gumbel searches begun, halvings made) since agz_selfplay_start
function gumbel_counts(e::Engine)
  out = zeros(Int64, 2)
  check(e, ccall((:agz_selfplay_gumbel_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{Int64}), e.handle, out))
  Int(out[1]), Int(out[2])
end
# the improved-policy row of node `node` of single tree g under the constants given, whatever the engine's setting
function gumbel_pi(e::Engine, g::Integer, node::Integer, c_visit::Real, c_scale::Real, A::Integer)
  out = zeros(Float32, A)
  check(e, ccall((:agz_tree_gumbel_pi, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Float64, Ptr{Float32}),
                 e.handle, g, node, c_visit, c_scale, out))
  out
end

# PUCT rule options (ours; include/agz.h agz_search_set_puct), for every search the engine runs.  fpu = nothing (off: an
# unvisited child's Q is 0), r, or (r, r_root): first-play urgency reduction -- an unvisited child's Q is its parent's
# value less r * sqrt(policy mass of the visited children), r_root at the game's root; fpu = 0.0 is not off.
# c_base > 0: c_puct grows by log((1 + N + c_base) / c_base) with the node's visits (AlphaZero: 19652); 0 is off.
function set_puct!(e::Engine, fpu = nothing, c_base::Real = 0.0)
  on = fpu === nothing ? 0 : 1
  r, r_root = fpu === nothing ? (0.0, 0.0) : fpu isa Tuple ? (fpu[1], fpu[2]) : (fpu, fpu)
  check(e, ccall((:agz_search_set_puct, libagz), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Float64), e.handle, on, r,
                 r_root, c_base))
end
# (tree levels scored under an active rule, those of them that picked an unvisited child) since the later of
# set_puct! and agz_selfplay_start
function puct_counts(e::Engine)
  out = zeros(UInt64, 2)
  check(e, ccall((:agz_search_puct_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{UInt64}), e.handle, out))
  Int(out[1]), Int(out[2])
end
# the keywords fpu = / c_base = of selfplay, train, analyze, review, evaluate and MCTSPlayer: nothing asked, nothing set
apply_puct!(e::Engine, fpu, c_base) = (fpu === nothing && c_base == 0) || set_puct!(e, fpu, c_base)

# Root exploration and the move temperature (ours; include/agz.h agz_selfplay_set_root_policy_temperature and what follows
# it, DESIGN.md 5t).  A temperature t is nothing (off), T, or (early, late, halflife): T(n) = late + (early - late) *
# 2^(-n / halflife), n = position.n of the root.  root policy temperature: the root prior of a search that gets noise is
# re-softmaxed at T(n) first; root noise: Dirichlet noise of total concentration total_alpha over the legal moves only
# (0: off, the reference's one alpha over all actions), each move's share shaped by the prior with shaped = true
# (KataGo); move temperature: pick_move (two_player_mode off) samples in proportion to N^(1 / T(n)), arg-max once
# T(n) <= 0.01.
schedule_args(t) = t === nothing ? (Int32(0), 1.0, 1.0, 1.0) :
                   t isa Tuple ? (Int32(1), Float64(t[1]), Float64(t[2]), Float64(t[3])) : (Int32(1), Float64(t), Float64(t), 1.0)
function set_root_policy_temperature!(e::Engine, t = nothing)
  on, early, late, half = schedule_args(t)
  check(e, ccall((:agz_selfplay_set_root_policy_temperature, libagz), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Float64),
                 e.handle, on, early, late, half))
end
function set_root_noise!(e::Engine, total_alpha::Real = 0.0, shaped::Bool = false)
  check(e, ccall((:agz_selfplay_set_root_noise, libagz), Int32, (Ptr{Cvoid}, Float64, Int32), e.handle, total_alpha,
                 shaped ? 1 : 0))
end
function set_move_temperature!(e::Engine, t = nothing)
  on, early, late, half = schedule_args(t)
  check(e, ccall((:agz_search_set_move_temperature, libagz), Int32, (Ptr{Cvoid}, Int32, Float64, Float64, Float64),
                 e.handle, on, early, late, half))
end
# (roots tempered, roots noised under total_alpha > 0, moves sampled, those of them off the most visited child) since the
# later of a setter call and agz_selfplay_start
function explore_counts(e::Engine)
  out = zeros(UInt64, 4)
  check(e, ccall((:agz_search_explore_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{UInt64}), e.handle, out))
  Tuple(Int.(out))
end
# what inject_noise! would do to `node` of single tree g under the engine's setting: (tempered, alpha, noised); the tree
# is not modified
function explore_rows(e::Engine, g::Integer, node::Integer, A::Integer)
  t, al, nz = zeros(Float32, A), zeros(Float64, A), zeros(Float32, A)
  check(e, ccall((:agz_tree_explore_rows, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Ptr{Float64}, Ptr{Float32}),
                 e.handle, g, node, t, al, nz))
  t, al, nz
end
function explore_temperature(n::Integer, early::Real, late::Real, halflife::Real)
  out = Ref{Float64}(0.0)
  ccall((:agz_explore_temperature, libagz), Int32, (Int32, Float64, Float64, Float64, Ref{Float64}), n, early, late, halflife, out)
  out[]
end
# Value uncertainty (ours; include/agz.h agz_search_set_value_moments and what follows it, DESIGN.md 5w).  Moments: a sum
# of squared values S beside every W.  lcb = nothing (off), z, or (z, min_visits, min_ratio): the arg-max branch of pick_move
# takes the largest lower confidence bound among the well-visited children.  puct_variance = nothing (off), k, or (k,
# prior, prior_weight): the PUCT scale times 1 + k * (sd / prior - 1) of the node's own values.
function set_value_moments!(e::Engine, on::Bool = true)
  check(e, ccall((:agz_search_set_value_moments, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, on ? 1 : 0))
end
function set_lcb!(e::Engine, lcb = nothing)
  z, mv, ratio = lcb === nothing ? (0.0, 1, 0.0) : lcb isa Tuple ? (lcb[1], lcb[2], lcb[3]) : (lcb, 1, 0.0)
  check(e, ccall((:agz_search_set_lcb, libagz), Int32, (Ptr{Cvoid}, Float64, Int32, Float64), e.handle, z, mv, ratio))
end
function set_puct_variance!(e::Engine, pv = nothing)
  k, prior, weight = pv === nothing ? (0.0, 0.4, 2.0) : pv isa Tuple ? (pv[1], pv[2], pv[3]) : (pv, 0.4, 2.0)
  check(e, ccall((:agz_search_set_puct_variance, libagz), Int32, (Ptr{Cvoid}, Float64, Float64, Float64), e.handle, k, prior,
                 weight))
end
# (moves picked under the LCB rule, those off the most visited child, levels scored under a variance factor, those with
# factor > 1) since the later of a setter call and agz_selfplay_start
function uncertainty_counts(e::Engine)
  out = zeros(UInt64, 4)
  check(e, ccall((:agz_search_uncertainty_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{UInt64}), e.handle, out))
  Tuple(Int.(out))
end
# (mean, sd, lcb) of the children of `node` of single tree g under z, from the node's side to move
function child_lcb(e::Engine, g::Integer, node::Integer, z::Real, A::Integer)
  m, sd, l = zeros(Float64, A), zeros(Float64, A), zeros(Float64, A)
  check(e, ccall((:agz_tree_child_lcb, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Float64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                 e.handle, g, node, z, m, sd, l))
  m, sd, l
end
function node_S(e::Engine, g::Integer, node::Integer)
  out = Ref{Float32}(0.0f0)
  check(e, ccall((:agz_tree_node_S, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ref{Float32}), e.handle, g, node, out))
  out[]
end
# (child_S [A, rows], root_S [rows]) of the analysis / review run, which began with moments on
function analyze_child_S(e::Engine, rows::Integer, A::Integer)
  cs, rs = zeros(Float32, A, rows), zeros(Float32, rows)
  check(e, ccall((:agz_analyze_child_S, libagz), Int32, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), e.handle, cs, rs))
  cs, rs
end
function value_lcb(n::Real, w::Real, s::Real, to_play::Integer, z::Real)
  m, sd, l = Ref{Float64}(0.0), Ref{Float64}(0.0), Ref{Float64}(0.0)
  ccall((:agz_value_lcb, libagz), Int32, (Float32, Float32, Float32, Int32, Float64, Ref{Float64}, Ref{Float64}, Ref{Float64}),
        n, w, s, to_play, z, m, sd, l)
  m[], sd[], l[]
end
function puct_variance_factor(n::Real, w::Real, s::Real, k::Real, prior::Real, weight::Real)
  out = Ref{Float64}(0.0)
  ccall((:agz_puct_variance_factor, libagz), Int32, (Float32, Float32, Float32, Float64, Float64, Float64, Ref{Float64}),
        n, w, s, k, prior, weight, out)
  out[]
end
# the keywords lcb = / puct_variance = of selfplay, train, analyze, review, evaluate and MCTSPlayer: either switches the
# moments on; nothing asked, nothing set
function apply_uncertainty!(e::Engine, lcb, puct_variance)
  (lcb === nothing && puct_variance === nothing) && return nothing
  set_value_moments!(e, true)
  lcb === nothing || set_lcb!(e, lcb)
  puct_variance === nothing || set_puct_variance!(e, puct_variance)
  nothing
end

# Superko (ours; include/agz.h agz_search_set_ko_rule and what follows it, include/agz_superko.h, DESIGN.md 5x): beside the
# simple ko, a move that recreates a position the game has seen is refused -- :positional the board alone, :situational
# the board with the side to move; :simple (the default) is the engine as it was.
const KO_RULES = Dict(:simple => Int32(0), :positional => Int32(1), :situational => Int32(2))
ko_rule_number(rule) = rule === nothing ? Int32(0) : rule isa Integer ? Int32(rule) : KO_RULES[Symbol(rule)]
function set_ko_rule!(e::Engine, rule = :simple)
  check(e, ccall((:agz_search_set_ko_rule, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, ko_rule_number(rule)))
end
# (nodes that lost at least one move to the rule, moves removed)
function superko_counts(e::Engine)
  out = zeros(UInt64, 2)
  check(e, ccall((:agz_search_superko_counts, libagz), Int32, (Ptr{Cvoid}, Ptr{UInt64}), e.handle, out))
  (Int(out[1]), Int(out[2]))
end
function node_key(e::Engine, g::Integer, node::Integer)
  out = Ref{UInt64}(0)
  check(e, ccall((:agz_tree_node_key, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt64}), e.handle, g, node, out))
  out[]
end
function node_legal(e::Engine, g::Integer, node::Integer, A::Integer)
  out = zeros(Int8, A)
  check(e, ccall((:agz_tree_node_legal, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Int8}), e.handle, g, node, out))
  out
end
# the keys of B positions (boards Int8 [P, B], to_play Int8 [B]) under `rule`
function position_keys(e::Engine, boards::Matrix{Int8}, to_play::Vector{Int8}, rule = :positional)
  out = zeros(UInt64, length(to_play))
  check(e, ccall((:agz_go_keys, libagz), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Int32, Int32, Ptr{UInt64}), e.handle,
                 boards, to_play, length(to_play), ko_rule_number(rule), out))
  out
end
# all_legal_moves under `rule`; seen: one vector of keys per position
function legal_moves_seen(e::Engine, boards::Matrix{Int8}, to_play::Vector{Int8}, ko::Vector{Int32}, seen, A::Integer,
                          rule = :positional)
  B = length(to_play)
  off = Int64[0; cumsum(length.(seen))]
  flat = UInt64[k for s in seen for k in s]
  push!(flat, 0)
  out = zeros(Int8, A, B)
  check(e, ccall((:agz_go_legal_seen, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{UInt64}, Ptr{Int64}, Int32, Int32, Ptr{Int8}), e.handle,
                 boards, to_play, ko, flat, off, B, ko_rule_number(rule), out))
  out
end
# host only, no engine
function position_key(board::Vector{Int8}, to_play::Integer, rule = :positional)
  out = Ref{UInt64}(0)
  st = ccall((:agz_go_position_key, libagz), Int32, (Ptr{Int8}, Int32, Int32, Int32, Ptr{UInt64}), board, length(board),
             to_play, ko_rule_number(rule), out)
  st == 0 || error("position_key: to_play is +-1, rule one of :simple, :positional, :situational")
  out[]
end
# the keyword ko_rule = of selfplay, train, analyze, review, evaluate and MCTSPlayer: nothing asked, nothing set
apply_ko_rule!(e::Engine, ko_rule) = ko_rule === nothing ? nothing : set_ko_rule!(e, ko_rule)

# the keywords root_policy_temperature = / root_noise = (total_alpha, shaped) / move_temperature = of selfplay, train and
# MCTSPlayer (analyze and review take move_temperature): nothing asked, nothing set
function apply_explore!(e::Engine, root_policy_temperature, root_noise, move_temperature)
  root_policy_temperature === nothing || set_root_policy_temperature!(e, root_policy_temperature)
  root_noise === nothing || (root_noise isa Tuple ? set_root_noise!(e, root_noise[1], root_noise[2]) : set_root_noise!(e, root_noise))
  move_temperature === nothing || set_move_temperature!(e, move_temperature)
  nothing
end

# replay_position (board.jl:557-578) from a start position: the position before each move and the final one
function replay_positions_from(start::Position, moves)
  positions = Position[]
  pos = start
  for m in moves
    push!(positions, pos)
    pos = play_move!(pos, m)
  end
  positions, pos
end

function selfplay(env::GoEnv, nn::NeuralNet, num_ro::Int = 800; games::Union{Nothing, Int} = nothing,
                  slots::Union{Nothing, Int} = nothing, seed = nothing, game_id_base = nothing, symmetry = nothing,
                  starts::Union{Nothing, Vector{Position}} = nothing, playout_cap = nothing,
                  forced_playouts = nothing, prune_targets::Bool = true,
                  gumbel = nothing, gumbel_c_visit::Real = 50.0, gumbel_c_scale::Real = 1.0,
                  fpu = nothing, c_base::Real = 0.0, root_policy_temperature = nothing, root_noise = nothing,
                  move_temperature = nothing)
  (gumbel !== nothing && gumbel != 0 && forced_playouts !== nothing && forced_playouts != 0) &&
    throw(ArgumentError("gumbel and forced_playouts are two rules for the same decision: ask for one"))
  G = games === nothing ? 1 : games
  if seed === nothing
    seed, next = STREAM[]
    if game_id_base === nothing
      game_id_base = next
      STREAM[] = (seed, next + UInt64(G))
    end
  end
  game_id_base === nothing && (game_id_base = 0)
  e = Engine(board_size = env.N, tower_height = nn.tower_height, games = slots === nothing ? min(G, 1024) : slots,
             num_readouts = num_ro, seed = seed, game_id_base = game_id_base, record_capacity_games = G + 8)
  copy_weights!(e, nn.engine)
  symmetry === nothing || set_symmetry!(e, symmetry)
  starts === nothing || set_starts!(e, env, starts)
  playout_cap === nothing || set_playout_cap!(e, playout_cap[1], playout_cap[2])      # (r, p)
  forced_playouts === nothing || set_forced_playouts!(e, forced_playouts, prune_targets)   # k
  gumbel === nothing || set_gumbel!(e, gumbel, gumbel_c_visit, gumbel_c_scale)             # m
  apply_puct!(e, fpu, c_base)                                                              # the PUCT rule options
  apply_explore!(e, root_policy_temperature, root_noise, move_temperature)                 # root exploration, move temperature
  check(e, ccall((:agz_selfplay_start, libagz), Int32, (Ptr{Cvoid}, Int64), e.handle, G))
  while ccall((:agz_records_count, libagz), Int64, (Ptr{Cvoid},), e.handle) < G
    check(e, ccall((:agz_selfplay_step, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 16))
    check_pool(e)     # a game whose node pool ran out cannot finish: raise instead of stepping for ever
  end
  players = SelfPlayPlayer[]
  A = env.action_space
  τ = (env.N * env.N ÷ 12) ÷ 2 * 2
  for k in 0:G-1
    h = Ref{AgzGameHeader}()
    check(e, ccall((:agz_records_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
    n = Int(h[].num_moves)
    moves = zeros(Int16, max(n, 1)); pis = zeros(Float32, A, max(n, 1)); qs = zeros(Float32, max(n, 1))
    check(e, ccall((:agz_records_game, libagz), Int32, (Ptr{Cvoid}, Int64, Ptr{Int16}, Ptr{Float32}, Ptr{Float32}),
                   e.handle, k, moves, pis, qs))
    rs = h[].was_resign != 0 ? (h[].result == BLACK ? "B+R" : "W+R") : result_string(h[].final_score)
    fmoves = Int.(moves[1:n]) .+ 1
    recent, color = PlayerMove[], BLACK
    for f in fmoves
      push!(recent, PlayerMove(color, from_flat(f, env))); color = -color
    end
    si = starts === nothing || isempty(starts) ? -1 : Int(h[].game_id % UInt64(length(starts)))
    positions, final = si < 0 ? replay_positions(env, 7.5, recent) :
                                replay_positions_from(starts[si + 1], [from_flat(f, env) for f in fmoves])
    push!(players, SelfPlayPlayer(env, nn, num_ro, false, τ, qs[1:n], [pis[:, i] for i in 1:n], Int(h[].result), rs,
                                  FinishedRoot(final), h[].resign_disabled != 0 ? -1.0 : -0.9, final, positions,
                                  h[].game_id, fmoves, Int(h[].short_searches), si < 0 ? nothing : starts[si + 1], si,
                                  Bool[any(!iszero, view(pis, :, i)) for i in 1:n]))
  end
  sort!(players, by = r -> r.game_id)
  games === nothing ? players[1] : players
end

# analyze(env, nn, positions; num_readouts) (ours): suggest_move over many positions in one device run.  Result i is what
# MCTSPlayer(env, nn; num_readouts, two_player_mode) with draw-stream seed `seed` and game id game_id_base + i - 1,
# initialize_game!(player, positions[i]) and suggest_move(player) compute, bit for bit (include/agz.h agz_analyze_start).
# Each result is a NamedTuple: move (board coordinates, nothing for a pass or when no move was picked), N, W, Q of the
# root, child_N / child_W / child_Q / child_prior (length A), status (AGZ_OK, AGZ_BAD_ARGUMENT for an invalid board,
# AGZ_POOL_EXHAUSTED, AGZ_ASSERT_SOFTPICK) and nodes_used.
function analyze(env::GoEnv, nn::NeuralNet, positions::Vector{Position}; num_readouts::Int = 800, seed = 0,
                 game_id_base = 0, slots::Union{Nothing, Int} = nothing, two_player_mode = false, symmetry = nothing,
                 lines::Int = 0, pv_depth::Int = 16, pv_min_visits::Int = 1, fpu = nothing, c_base::Real = 0.0,
                 move_temperature = nothing)
  check_lines(lines, pv_depth, pv_min_visits)
  B, P, A = length(positions), env.N * env.N, env.action_space
  B == 0 && return NamedTuple[]
  boards = zeros(Int8, P, B); hist = zeros(Int8, P, 7, B); info = Vector{AgzPositionInfo}(undef, B)
  for (i, pos) in enumerate(positions)
    b, info[i], h = position_arrays(env, pos)
    boards[:, i] = vec(b); hist[:, 1:size(h, 2), i] = h
  end
  # one search per tree, no re-rooting: a tree holds at most 1 + R + 2 parallel_readouts nodes
  e = Engine(board_size = env.N, tower_height = nn.tower_height, games = slots === nothing ? min(B, 1024) : slots,
             num_readouts = num_readouts, seed = seed, two_player_mode = two_player_mode,
             max_nodes_per_game = 2 * num_readouts + 256)
  copy_weights!(e, nn.engine)
  symmetry === nothing || set_symmetry!(e, symmetry)
  apply_puct!(e, fpu, c_base)
  apply_explore!(e, nothing, nothing, move_temperature)      # pick_move's, as MCTSPlayer(move_temperature = )
  lines > 0 && check(e, ccall((:agz_analyze_set_lines, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32),
                              e.handle, lines, pv_depth, pv_min_visits))
  check(e, ccall((:agz_analyze_start, libagz), Int32, (Ptr{Cvoid}, Ptr{Int8}, Ptr{AgzPositionInfo}, Ptr{Int8}, Int64, UInt64),
                 e.handle, boards, info, hist, B, game_id_base))
  done = Ref{Int64}(0)
  while true
    check(e, ccall((:agz_analyze_progress, libagz), Int32, (Ptr{Cvoid}, Ref{Int64}), e.handle, done))
    done[] >= B && break
    check(e, ccall((:agz_selfplay_step, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 16))
    check_pool(e)     # a search waiting on a full pool (AGZ_POOL_STALL) cannot finish
  end
  res = Vector{AgzAnalysis}(undef, B)
  cn, cw, pr = zeros(Float32, A, B), zeros(Float32, A, B), zeros(Float32, A, B)
  check(e, ccall((:agz_analyze_results, libagz), Int32, (Ptr{Cvoid}, Ptr{AgzAnalysis}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                 e.handle, res, cn, cw, pr))
  rows = [(move = r.move < 0 ? nothing : from_flat(r.move + 1, env), N = r.N, W = r.W, Q = r.Q, child_N = cn[:, i],
           child_W = cw[:, i], child_Q = cw[:, i] ./ (1f0 .+ cn[:, i]), child_prior = pr[:, i], status = Int(r.status),
           nodes_used = Int(r.nodes_used)) for (i, r) in enumerate(res)]
  lines > 0 || return rows
  ln, pv, pvn = read_lines(e, B, lines, pv_depth)
  [merge(rows[i], (lines = line_rows(env, ln[:, i], pv[:, :, i], pvn[:, :, i]),)) for i in 1:B]
end

function check_lines(lines, pv_depth, pv_min_visits)
  0 <= lines <= 16 || throw(ArgumentError("lines must be in 0..16"))
  1 <= pv_depth <= 64 || throw(ArgumentError("pv_depth must be in 1..64"))
  pv_min_visits >= 1 || throw(ArgumentError("pv_min_visits must be >= 1"))
end
# the lines tables of a finished analysis / review run: lines K x rows, pv and pv_N D x K x rows
function read_lines(e, rows, K, D)
  ln = Matrix{AgzLine}(undef, K, rows); pv = zeros(Int16, D, K, rows); pvn = zeros(Float32, D, K, rows)
  check(e, ccall((:agz_analyze_lines, libagz), Int32, (Ptr{Cvoid}, Ptr{AgzLine}, Ptr{Int16}, Ptr{Float32}),
                 e.handle, ln, pv, pvn))
  ln, pv, pvn
end

# review(env, nn, games; num_readouts) (ours): the loop of play() (src/play.jl:25-77) over recorded games in one device
# run.  games[j] is a SelfPlayPlayer or a move list (board coordinates, nothing = pass, or 1-based flat moves); starts is
# nothing (the empty board) or one Position per game.  Result j is a vector of the NamedTuples analyze returns, entry k
# what MCTSPlayer(env, nn; num_readouts, two_player_mode) with draw-stream seed `seed` and game id game_id_base + j - 1,
# initialize_game!(player, starts[j]) and then suggest_move(player) / play_move!(player, m_k) compute at its k-th
# suggest_move, bit for bit (include/agz.h agz_review_start).  A recorded move that cannot be played gives its ply and
# the later ones of that game status AGZ_BAD_ARGUMENT.
function review(env::GoEnv, nn::NeuralNet, games::Vector; num_readouts::Int = 800, starts = nothing,
                two_player_mode = true, seed = 0, game_id_base = 0, slots::Union{Nothing, Int} = nothing,
                symmetry = nothing, lines::Int = 0, pv_depth::Int = 16, pv_min_visits::Int = 1, fpu = nothing,
                c_base::Real = 0.0, move_temperature = nothing)
  check_lines(lines, pv_depth, pv_min_visits)
  G, P, A = length(games), env.N * env.N, env.action_space
  G == 0 && return Vector{NamedTuple}[]
  num_readouts >= 1 || throw(ArgumentError("num_readouts must be >= 1"))
  moves = Int16[]; off = Int64[0]
  for g in games
    seq = g isa SelfPlayPlayer ? g.moves : g
    for m in seq
      f = m === nothing ? P + 1 : m isa Integer ? Int(m) : to_flat(m, env)
      1 <= f <= P + 1 || throw(ArgumentError("move $m is not on the $(env.N)x$(env.N) board"))
      push!(moves, Int16(f - 1))
    end
    push!(off, length(moves))
  end
  boards = C_NULL; info = C_NULL; hist = C_NULL
  if starts !== nothing
    length(starts) == G || throw(ArgumentError("$(length(starts)) starts for $G games"))
    boards = zeros(Int8, P, G); hist = zeros(Int8, P, 7, G); info = Vector{AgzPositionInfo}(undef, G)
    for (j, pos) in enumerate(starts)
      b, info[j], h = position_arrays(env, pos === nothing ? Position(env) : pos)
      boards[:, j] = vec(b); hist[:, 1:size(h, 2), j] = h
    end
  end
  # trees are re-rooted and kept, as in self-play: the engine's default pool
  e = Engine(board_size = env.N, tower_height = nn.tower_height, games = slots === nothing ? min(G, 1024) : slots,
             num_readouts = num_readouts, seed = seed, two_player_mode = two_player_mode)
  copy_weights!(e, nn.engine)
  symmetry === nothing || set_symmetry!(e, symmetry)
  apply_puct!(e, fpu, c_base)
  apply_explore!(e, nothing, nothing, move_temperature)      # pick_move's, as MCTSPlayer(move_temperature = )
  lines > 0 && check(e, ccall((:agz_analyze_set_lines, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32),
                              e.handle, lines, pv_depth, pv_min_visits))
  check(e, ccall((:agz_review_start, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int16}, Ptr{Int64}, Ptr{Int8}, Ptr{AgzPositionInfo}, Ptr{Int8}, Int64, UInt64),
                 e.handle, moves, off, boards, info, hist, G, game_id_base))
  review_rows(e, env, off, UInt64[UInt64(game_id_base + j - 1) for j in 1:G], lines, pv_depth)
end

# the loop behind review and reanalyze!: step the review run on `e` until its off[end] rows are finished, then read them
# as one vector of NamedTuples per game (game j's rows off[j]+1 .. off[j+1], its game id ids[j])
function review_rows(e::Engine, env::GoEnv, off::Vector{Int64}, ids::Vector{UInt64}, lines::Int, pv_depth::Int)
  G, A, total = length(ids), env.action_space, off[end]
  done = Ref{Int64}(0)
  while true
    check(e, ccall((:agz_analyze_progress, libagz), Int32, (Ptr{Cvoid}, Ref{Int64}), e.handle, done))
    done[] >= total && break
    check(e, ccall((:agz_selfplay_step, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 16))
    check_pool(e)     # a search waiting on a full pool (AGZ_POOL_STALL) cannot finish
  end
  res = Vector{AgzAnalysis}(undef, total)
  cn, cw, pr = zeros(Float32, A, total), zeros(Float32, A, total), zeros(Float32, A, total)
  check(e, ccall((:agz_analyze_results, libagz), Int32, (Ptr{Cvoid}, Ptr{AgzAnalysis}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                 e.handle, res, cn, cw, pr))
  row(i, id) = (r = res[i]; (move = r.move < 0 ? nothing : from_flat(r.move + 1, env), N = r.N, W = r.W, Q = r.Q,
            child_N = cn[:, i], child_W = cw[:, i], child_Q = cw[:, i] ./ (1f0 .+ cn[:, i]), child_prior = pr[:, i],
            status = Int(r.status), nodes_used = Int(r.nodes_used), game_id = id))
  ln, pv, pvn = lines > 0 ? read_lines(e, total, lines, pv_depth) : (nothing, nothing, nothing)
  withlines(i, r) = lines > 0 ? merge(r, (lines = line_rows(env, ln[:, i], pv[:, :, i], pvn[:, :, i]),)) : r
  out = Vector{Vector{NamedTuple}}(undef, G)
  for j in 1:G
    out[j] = [withlines(i, row(i, ids[j])) for i in off[j]+1:off[j+1]]
  end
  out
end

# reanalyze!(e, env; first, count) (ours; MuZero's Reanalyse, include/agz.h agz_replay_reanalyze_start / _commit): search
# the replay-arena games first .. first + count - 1 (0-based, count = nothing: all from `first`) of engine `e` again on
# its current network -- a review run gathered on the device, game id game_id_base + the record's -- and, with commit,
# write every finished row over its record: qs[k] = Q, and the new π row unless the old one is all zero.  Moves, results
# and the arena's order stay.  Returns ((committed, pi_rows, skipped) or nothing, the rows per game as review gives them).
function reanalyze!(e::Engine, env::GoEnv; first::Integer = 0, count::Union{Nothing, Integer} = nothing, game_id_base = 0,
                    commit::Bool = true, lines::Int = 0, pv_depth::Int = 16, pv_min_visits::Int = 1)
  check_lines(lines, pv_depth, pv_min_visits)
  G = count === nothing ? replay_games(e) - first : count
  check(e, ccall((:agz_analyze_set_lines, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Int32),
                 e.handle, lines, pv_depth, pv_min_visits))
  check(e, ccall((:agz_replay_reanalyze_start, libagz), Int32, (Ptr{Cvoid}, Int64, Int64, UInt64),
                 e.handle, first, G, game_id_base))
  h = Ref{AgzGameHeader}()
  off = Int64[0]; ids = UInt64[]
  for k in first:first+G-1
    check(e, ccall((:agz_replay_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
    push!(off, off[end] + h[].num_moves); push!(ids, UInt64(game_id_base) + h[].game_id)
  end
  rows = review_rows(e, env, off, ids, lines, pv_depth)
  commit || return nothing, rows
  counts = zeros(Int64, 3)
  check(e, ccall((:agz_replay_reanalyze_commit, libagz), Int32, (Ptr{Cvoid}, Ptr{Int64}), e.handle, counts))
  (committed = counts[1], pi_rows = counts[2], skipped = counts[3]), rows
end

# get_replay_batch(pos_buffer, π_buffer, res_buffer; batch_size), src/train.jl:4-12: batch_size distinct entries,
# π as an A x B matrix
function get_replay_batch(pos_buffer::Vector{Position}, π_buffer, res_buffer; batch_size = 32)
  picks = randperm(length(pos_buffer))[1:batch_size]             # sample(1:n, batch_size, replace = false)
  pos_buffer[picks], reduce(hcat, π_buffer[picks]), res_buffer[picks]
end

# _train(nn, (positions, π, z), opt; epochs), src/neural_net.jl:85-101 (call: train.jl:70) as intended -- the
# reference's does not run at HEAD (SURVEY.md D3): minibatches of 32 positions, each ONE agz_train_step on the device
# (training-mode forward, 0.01 crossentropy + 0.01 mse + 1e-4 sum(θ²), backward, Momentum update of nn in place).
# Returns the summed minibatch loss / epochs (:98-100).  Momentum(η, ρ = 0.9) stands for Flux.Momentum (train.jl:54):
# its velocity lives in the network's engine.
struct Momentum
  eta::Float32
  rho::Float32
end
Momentum(eta = 0.01f0) = Momentum(eta, 0.9f0)

function _train(nn::NeuralNet, input_data, opt::Momentum; epochs = 1)
  positions, π, z = input_data
  env = nn.env; N = env.N; n = length(positions)
  boards = cat(dims = 3, (p.board for p in positions)...)
  deltas = zeros(Int8, N, N, 7, n); nd = zeros(Int32, n)
  for (b, p) in enumerate(positions)
    k = size(p.board_deltas, 3); nd[b] = k
    deltas[:, :, 1:k, b] .= p.board_deltas
  end
  tp = Int8[p.to_play for p in positions]
  feats = zeros(Float32, N * N * 17, n)
  check(nn.engine, ccall((:agz_features, libagz), Int32,
        (Ptr{Cvoid}, Ptr{Int8}, Ptr{Int8}, Ptr{Int32}, Ptr{Int8}, Int32, Ptr{Float32}),
        nn.engine.handle, boards, deltas, nd, tp, n, feats))
  cuts = vcat(collect(1:32:n), n + 1)
  length(cuts) > 2 && cuts[end] - cuts[end-1] == 1 && deleteat!(cuts, length(cuts) - 1)   # BatchNorm needs two rows
  loss_avg = 0f0
  for _ in 1:epochs, j in 1:length(cuts)-1
    r = cuts[j]:cuts[j+1]-1
    loss_avg += train_step!(nn.engine, feats[:, r], Matrix{Float32}(π[:, r]), Float32.(z[r]); eta = opt.eta, rho = opt.rho)[1]
  end
  loss_avg / epochs
end

# every (layer, kind) of a network with `t` residual blocks (ids as in include/agz.h)
function layer_kinds(t::Integer)
  lk = Tuple{Int32, Int32}[]
  for l in vcat(collect(0:2t), [-1, -2]), k in 0:6
    push!(lk, (l, k))
  end
  for l in (-3, -4, -5), k in 0:1
    push!(lk, (l, k))
  end
  lk
end

function copy_weights!(dst::Engine, src::Engine)
  for (l, k) in layer_kinds(src.cfg.tower_height)
    n = ccall((:agz_net_param_count, libagz), Int64, (Ptr{Cvoid}, Int32, Int32), src.handle, l, k)
    buf = zeros(Float32, n)
    check(src, ccall((:agz_net_get_weights, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Int64),
                     src.handle, l, k, buf, n))
    check(dst, ccall((:agz_net_set_weights, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Int64),
                     dst.handle, l, k, buf, n))
  end
  dst
end

# tower arithmetic of an engine's network: :f32 (default, exact) or :f16 (fp16 operands, f32 accumulate)
# the f32 Winograd tower as one persistent launch (same bits as one launch per layer, include/agz.h)
set_tower_persistent!(e::Engine, on::Bool) =
  check(e, ccall((:agz_net_set_tower_persistent, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, on ? 1 : 0))
# the F(4x4,3x3) tower (boards >= 13x13) as two independent layer chains on two streams (default) or one
set_tower_streams!(e::Engine, n::Integer) =
  check(e, ccall((:agz_net_set_tower_streams, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, n))
set_precision!(e::Engine, p::Symbol) =      # :f32 (default, exact), :f16 (fp16 operands), :f32s (f32 as split f16 operands)
  check(e, ccall((:agz_net_set_precision, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, p === :f16 ? 1 : p === :f32s ? 2 : 0))

# ------------------------------------------------------------------ evaluate
# evaluate(env, black_net, white_net; num_games, ro), src/neural_net.jl:103-158: both networks live
# in one arena_mode engine (network 0 = Black's, 1 = White's), every game is a pair of slots, all
# games run concurrently.  Black's tally is `result(black.root.position) == BLACK` (:147), i.e.
# final_score > 0, also for resigned games.
function evaluate(env::GoEnv, black_net::NeuralNet, white_net::NeuralNet; num_games = 400, ro = 800,
                  verbose::Bool = false, seed = 0, pairs::Int = min(num_games, 512), symmetry = nothing,
                  starts::Union{Nothing, Vector{Position}} = nothing, fpu = nothing, c_base::Real = 0.0)
  @assert black_net.tower_height == white_net.tower_height
  e = Engine(board_size = env.N, tower_height = black_net.tower_height, games = 2 * pairs, num_readouts = ro,
             seed = seed, record_capacity_games = num_games + 8, arena_mode = true)
  copy_weights!(e, black_net.engine)
  check(e, ccall((:agz_net_select, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 1))
  copy_weights!(e, white_net.engine)
  check(e, ccall((:agz_net_select, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 0))
  symmetry === nothing || set_symmetry!(e, symmetry)
  apply_puct!(e, fpu, c_base)                            # both players
  starts === nothing || set_starts!(e, env, starts)      # an opening suite: game g begins at starts[g % S + 1]
  check(e, ccall((:agz_selfplay_start, libagz), Int32, (Ptr{Cvoid}, Int64), e.handle, num_games))
  while ccall((:agz_records_count, libagz), Int64, (Ptr{Cvoid},), e.handle) < num_games
    check(e, ccall((:agz_selfplay_step, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 16))
    check_pool(e)
  end
  games_won = 0
  for k in 0:num_games-1
    h = Ref{AgzGameHeader}()
    check(e, ccall((:agz_records_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
    games_won += h[].final_score > 0
  end
  verbose && print("Won $games_won / $num_games. Win rate: $(games_won/num_games). ")
  return games_won / num_games ≥ 0.55
end

# ------------------------------------------------------------------ replay batches
# get_replay_batch(pos_buffer, π_buffer, res_buffer; batch_size), src/train.jl:4-12, with the
# positions kept as move lists: `games[g]` is a SelfPlayPlayer, a sample is (g, ply) with ply = 0 the
# empty board -- or, for games played from a table of start positions (selfplay(...; starts)), the game's start: `e`
# must have the same table set (set_starts!).  Returns the N x N x 17 x B feature tensor get_feats would build, π (A x B),
# results.
function get_replay_batch(e::Engine, env::GoEnv, games::Vector{SelfPlayPlayer}, samples::Vector{Tuple{Int,Int}})
  used = sort(unique(first.(samples)))
  offs = Dict{Int,Int32}(); moves = Int16[]
  for g in used
    offs[g] = length(moves)
    append!(moves, Int16.(games[g].moves .- 1))
  end
  B = length(samples)
  off = Int32[offs[g] for (g, _) in samples]; ply = Int32[j for (_, j) in samples]
  feats = zeros(Float32, env.N, env.N, 17, B)
  start = Int32[games[g].start_index for (g, _) in samples]
  check(e, ccall((:agz_replay_features_starts, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int16}, Int64, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Float32}, Int32),
                 e.handle, moves, length(moves), off, ply, start, B, feats, 0))
  π = hcat((games[g].searches_π[j + 1] for (g, j) in samples)...)
  feats, π, [games[g].result for (g, _) in samples]
end

# ---- replay arena, RCCL exchange and the training step (train.jl:47-74; SURVEY.md 8e, 8f rows 1 and 4)
# Every rank's finished games are all-gathered by libagz itself (RCCL over xGMI, device to device) into a
# device-resident replay arena; (game, ply) samples become (features, pi, z) on the device; one call is one
# optimisation step of _train.  The 128-byte communicator id is generated on rank 0 and handed to the other
# ranks by the host (Distributed.jl, MPI.jl, a shared file -- the library does not care).

comm_unique_id() = (id = zeros(UInt8, 128);
                    st = ccall((:agz_comm_unique_id, libagz), Int32, (Ptr{UInt8},), id);
                    st == AGZ_OK || error("libagz status $st: " * unsafe_string(ccall((:agz_last_error, libagz), Cstring, (Ptr{Cvoid},), C_NULL)));
                    id)

function comm_create(e::Engine, rank::Integer, world::Integer, id::Vector{UInt8})
  c = Ref{Ptr{Cvoid}}(C_NULL)
  check(e, ccall((:agz_comm_create, libagz), Int32, (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ref{Ptr{Cvoid}}),
                 e.handle, rank, world, id, c))
  c[]
end
comm_destroy(c::Ptr{Cvoid}) = ccall((:agz_comm_destroy, libagz), Cvoid, (Ptr{Cvoid},), c)

# push_data.(buffers, extract_data(player)) for the games of EVERY rank (train.jl:57-62); comm = C_NULL on one GPU
function allgather_records!(e::Engine, comm::Ptr{Cvoid} = C_NULL)
  added = Ref{Int64}(0)
  check(e, ccall((:agz_allgather_records, libagz), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}), e.handle, comm, added))
  check(e, ccall((:agz_records_clear, libagz), Int32, (Ptr{Cvoid},), e.handle))
  added[]
end
# The same exchange with the bytes carried by the HOST's communication library (MPI.jl, Distributed): `allgather` is any
# function that takes this rank's Vector and returns the concatenation of every rank's, rank order.  Everything but the
# two collectives is libagz: what this rank announces, the count check / chunk stride (agz_gather_plan: the function
# agz_allgather_records itself calls), the packed export, device-side indexing and compaction into the arena.
# A rank whose pack step fails still joins the count collective with {-1, status}: every rank errors together.
function allgather_records_hosted!(e::Engine, world::Integer, allgather::Function)
  nb = Ref{Int64}(0)
  st = ccall((:agz_records_packed_size, libagz), Int32, (Ptr{Cvoid}, Ref{Int64}), e.handle, nb)
  mine = st == AGZ_OK ? Int64[ccall((:agz_records_count, libagz), Int64, (Ptr{Cvoid},), e.handle), nb[]] : Int64[-1, st]
  counts = allgather(mine)::Vector{Int64}                                        # 2 x Int64 per rank
  stride = Ref{Int64}(0); total = Ref{Int64}(0)
  pst = ccall((:agz_gather_plan, libagz), Int32, (Ptr{Int64}, Int32, Ref{Int64}, Ref{Int64}), counts, world, stride, total)
  st == AGZ_OK || check(e, st)
  pst == AGZ_OK || error("libagz status $pst: " * unsafe_string(ccall((:agz_last_error, libagz), Cstring, (Ptr{Cvoid},), C_NULL)))
  total[] == 0 && return 0
  send = zeros(UInt8, stride[])
  check(e, ccall((:agz_records_export_packed, libagz), Int32, (Ptr{Cvoid}, Ptr{UInt8}, Int64, Int32), e.handle, send, mine[2], 0))
  recv = allgather(send)::Vector{UInt8}                                          # world x stride bytes
  added = Ref{Int64}(0)
  check(e, ccall((:agz_replay_ingest_gathered, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{UInt8}, Int32, Int32, Int64, Ptr{Int64}, Ref{Int64}),
                 e.handle, recv, 0, world, stride[], counts, added))
  check(e, ccall((:agz_records_clear, libagz), Int32, (Ptr{Cvoid},), e.handle))
  added[]
end
broadcast_weights!(e::Engine, comm::Ptr{Cvoid}, root::Integer = 0) =
  check(e, ccall((:agz_broadcast_weights, libagz), Int32, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Ptr{Int64}), e.handle, comm, root, C_NULL))

replay_games(e::Engine) = ccall((:agz_replay_count, libagz), Int64, (Ptr{Cvoid},), e.handle)
replay_positions(e::Engine) = ccall((:agz_replay_positions, libagz), Int64, (Ptr{Cvoid},), e.handle)     # length(pos_buffer)
replay_trim!(e::Engine, memory_size::Integer) =                                                         # shrink, train.jl:52
  check(e, ccall((:agz_replay_trim, libagz), Int32, (Ptr{Cvoid}, Int64), e.handle, memory_size))
function replay_game_lengths(e::Engine)
  h = Ref{AgzGameHeader}()
  [begin
     check(e, ccall((:agz_replay_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
     Int(h[].num_moves)
   end for k in 0:replay_games(e)-1]
end

# get_replay_batch (train.jl:4-12): `games`/`plies` are 0-based (game index in the arena, move number);
# returns (feats N*N*17 x B, pi A x B, z B) -- column-major, i.e. exactly what `_train` consumes
function replay_batch(e::Engine, env::GoEnv, games::Vector{Int64}, plies::Vector{Int32})
  B = length(games)
  feats = zeros(Float32, env.N * env.N * 17, B); pi = zeros(Float32, env.action_space, B); z = zeros(Float32, B)
  check(e, ccall((:agz_replay_batch, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32),
                 e.handle, games, plies, B, feats, pi, z, 0))
  feats, pi, z
end

# the same with sample b under the board symmetry T_sym[b] (augmentation); augment = true draws one s per sample
function replay_batch(e::Engine, env::GoEnv, games::Vector{Int64}, plies::Vector{Int32}, sym::Vector{Int32})
  B = length(games)
  feats = zeros(Float32, env.N * env.N * 17, B); pi = zeros(Float32, env.action_space, B); z = zeros(Float32, B)
  check(e, ccall((:agz_replay_batch_sym, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32),
                 e.handle, games, plies, sym, B, feats, pi, z, 0))
  feats, pi, z
end
sample(e::Engine, env::GoEnv, games::Vector{Int64}, plies::Vector{Int32}; augment::Bool = false, rng = Random.default_rng()) =
  augment ? replay_batch(e, env, games, plies, Int32.(rand(rng, 0:7, length(games)))) : replay_batch(e, env, games, plies)

# _train(nn, (positions, pi, z), Momentum(2f-2)) for one batch (neural_net.jl:85-101): returns
# (total, policy, value, regulariser) losses before the update
function train_step!(e::Engine, feats::Matrix{Float32}, pi::Matrix{Float32}, z::Vector{Float32}; eta = 0.02f0, rho = 0.9f0)
  losses = zeros(Float32, 4)
  check(e, ccall((:agz_train_step, libagz), Int32,
                 (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Int32, Float32, Float32, Ptr{Float32}),
                 e.handle, feats, pi, z, length(z), 0, eta, rho, losses))
  Tuple(losses)
end

# train(env; num_games, memory_size, batch_size, epochs, ckp_freq, readouts, tower_height, model, start_training_after)
# (src/train.jl:38-92) with `slots` games in flight (DESIGN.md §5e; the Python mirror is api.train).  One engine plays,
# keeps the arena and trains; per step: agz_selfplay_step(1), one read of the finished games, and for each in game-id
# order: push_data (agz_replay_ingest_records, train.jl:60-61), shrink (agz_replay_set_window, :63-65), then _train on a
# device-drawn get_replay_batch (agz_replay_sample with draw key (seed, i), :67-70) in 32-position agz_train_step
# minibatches, Momentum(2f-2).  The hold keeps finished slots parked until agz_selfplay_release, so every game starts on
# the weights the games finished before it left; slots = 1 is the reference's loop.
function train(env::GoEnv; num_games::Int = 25000, memory_size::Int = 500000, batch_size::Int = 32, epochs = 1,
               ckp_freq::Int = 1000, readouts::Int = 800, tower_height::Int = 19, model = nothing,
               start_training_after = 50000, slots::Union{Nothing, Int} = nothing, seed = 0, game_id_base = 0,
               augment::Bool = false, callback::Function = println,
               starts::Union{Nothing, Vector{Position}} = nothing, playout_cap = nothing,
               forced_playouts = nothing, prune_targets::Bool = true,
               gumbel = nothing, gumbel_c_visit::Real = 50.0, gumbel_c_scale::Real = 1.0, value_target = nothing,
               fpu = nothing, c_base::Real = 0.0, surprise::Real = 0.0, root_policy_temperature = nothing,
               root_noise = nothing, move_temperature = nothing)
  (gumbel !== nothing && gumbel != 0 && forced_playouts !== nothing && forced_playouts != 0) &&
    throw(ArgumentError("gumbel and forced_playouts are two rules for the same decision: ask for one"))
  cur_nn = model === nothing ? NeuralNet(env; tower_height = tower_height) : model                       # train.jl:43
  S = slots === nothing ? min(num_games, 1024) : slots
  e = Engine(board_size = env.N, tower_height = cur_nn.tower_height, games = S, num_readouts = readouts, seed = seed,
             game_id_base = game_id_base, record_capacity_games = S + 8)
  copy_weights!(e, cur_nn.engine)
  opt = Momentum(2f-2)                                                                                     # train.jl:54
  P, A = env.N * env.N, env.action_space
  bufs = [Ref{Ptr{Cvoid}}(C_NULL) for _ in 1:3]
  for (r, n) in zip(bufs, (17 * P * batch_size, A * batch_size, batch_size))
    check(e, ccall((:agz_device_alloc, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{Ptr{Cvoid}}), e.handle, 4 * n, r))
  end
  feats, pi, z = (r[] for r in bufs)
  cuts = vcat(collect(0:32:batch_size-1), batch_size)
  length(cuts) > 2 && cuts[end] - cuts[end-1] == 1 && deleteat!(cuts, length(cuts) - 1)   # BatchNorm needs two rows
  starts === nothing || set_starts!(e, env, starts)      # game gid begins at starts[gid % S + 1]; the arena replays from there
  if playout_cap !== nothing      # (r, p): memory_size and start_training_after then count target entries (full searches)
    set_playout_cap!(e, playout_cap[1], playout_cap[2])
    replay_set_targets_only!(e, playout_cap[1] > 0)
  end
  forced_playouts === nothing || set_forced_playouts!(e, forced_playouts, prune_targets)   # k, as in selfplay
  gumbel === nothing || set_gumbel!(e, gumbel, gumbel_c_visit, gumbel_c_scale)             # m, as in selfplay
  apply_puct!(e, fpu, c_base)                                                              # as in selfplay
  apply_explore!(e, root_policy_temperature, root_noise, move_temperature)                 # as in selfplay
  value_target === nothing || replay_set_value_target!(e, value_target[1], value_target[2])   # (alpha, lam): z of the batches
  replay_set_surprise!(e, surprise)       # rho: each game is scored as it is filed, the batches are drawn by weight
  check(e, ccall((:agz_selfplay_set_hold, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 1))
  check(e, ccall((:agz_selfplay_start, libagz), Int32, (Ptr{Cvoid}, Int64), e.handle, num_games))
  check(e, ccall((:agz_selfplay_release, libagz), Int32, (Ptr{Cvoid},), e.handle))
  i = 0
  while i < num_games
    check(e, ccall((:agz_selfplay_step, libagz), Int32, (Ptr{Cvoid}, Int32), e.handle, 1))
    n = ccall((:agz_records_count, libagz), Int64, (Ptr{Cvoid},), e.handle)
    n == 0 && continue
    heads = Tuple{AgzGameHeader, Int64}[]
    for k in 0:n-1
      h = Ref{AgzGameHeader}()
      check(e, ccall((:agz_records_header, libagz), Int32, (Ptr{Cvoid}, Int64, Ref{AgzGameHeader}), e.handle, k, h))
      push!(heads, (h[], k))
    end
    sort!(heads, by = hk -> hk[1].game_id)
    for (h, k) in heads
      check(e, ccall((:agz_replay_ingest_records, libagz), Int32, (Ptr{Cvoid}, Int64, Int64, Ptr{Int64}),
                     e.handle, k, 1, C_NULL))                                                          # train.jl:60-61
      surprise > 0 && replay_score!(e, ccall((:agz_replay_count, libagz), Int64, (Ptr{Cvoid},), e.handle) - 1, 1)
      check(e, ccall((:agz_replay_set_window, libagz), Int32, (Ptr{Cvoid}, Int64), e.handle, memory_size))   # :63-65
      i += 1
      if ccall((:agz_replay_live_positions, libagz), Int64, (Ptr{Cvoid},), e.handle) >= start_training_after   # :67
        check(e, ccall((:agz_replay_sample, libagz), Int32,
                       (Ptr{Cvoid}, Int32, UInt64, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}),
                       e.handle, batch_size, i, augment ? 8 : -1, feats, pi, z, C_NULL, C_NULL))        # :68-69
        loss = 0f0
        losses = zeros(Float32, 4)
        for _ in 1:epochs, j in 1:length(cuts)-1                                                       # :70
          lo, B = cuts[j], cuts[j+1] - cuts[j]
          check(e, ccall((:agz_train_step, libagz), Int32,
                         (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Int32, Float32, Float32, Ptr{Float32}),
                         e.handle, Ptr{Float32}(feats) + 4 * 17 * P * lo, Ptr{Float32}(pi) + 4 * A * lo,
                         Ptr{Float32}(z) + 4 * lo, B, 1, opt.eta, opt.rho, losses))
          loss += losses[1]
        end
        rs = h.was_resign != 0 ? (h.result == BLACK ? "B+R" : "W+R") : result_string(h.final_score)
        callback("Episode $i over. Loss: $(loss / epochs). Winner: $rs. Moves: $(h.num_moves).")        # :71-73
      end
      # (checkpoints, train.jl:86-89: the Python mirror writes them; this stub has no BSON writer)
    end
    check(e, ccall((:agz_records_clear, libagz), Int32, (Ptr{Cvoid},), e.handle))
    check(e, ccall((:agz_selfplay_release, libagz), Int32, (Ptr{Cvoid},), e.handle))
  end
  copy_weights!(cur_nn.engine, e)
  for r in bufs
    check(e, ccall((:agz_device_free, libagz), Int32, (Ptr{Cvoid}, Ptr{Cvoid}), e.handle, r[]))
  end
  cur_nn                                                                                                    # :91
end

end # module
