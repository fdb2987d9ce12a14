function [waypoints,n_wp,plan_status,hops] = planRoutes(po,goals,prm,cell,margin,W,obstacles)
% Route planning ahead of a transition (no reference counterpart: DMPC has no global planner, an agent behind a wall of uncommanded vehicles parks).
% po: 3 x N (or 1 x 3 x N as randomTest returns it); goals: 3 x N_cmd, N_cmd <= N: the vehicles behind the commanded ones are the obstacles to go
% round; obstacles (3 x M, optional) adds further points.  prm: a dmpc_params_struct (its rmin, c, pmin, pmax set the blocked cells and the grid's box).
% cell: the planning grid's cell in metres; margin (default 0) widens rmin; W (default 4): waypoint slots per agent.
% waypoints (3 x W x N_cmd) and n_wp (1 x N_cmd) are what dmpc_mex('route', prm, po, waypoints, K_T_max, error_tol, capture, n_wp) takes;
% plan_status: 0 ok, 1 truncated (more corners than W, the goal took the last slot), 2 no way (the goal alone); hops: cells of the path, -1 no way.
po = reshape(po,3,[]); goals = reshape(goals,3,[]);
if nargin < 5, margin = []; end
if nargin < 6, W = []; end
if nargin < 7, obstacles = zeros(3,0); end
[waypoints,n_wp,plan_status,hops] = dmpc_mex('plan', prm, po, goals, cell, margin, W, reshape(obstacles,3,[]));
end
